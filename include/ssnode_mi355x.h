/*
 * ssnode_mi355x.h -- C ABI of libssnode.so (MI355X / gfx950 build).
 *
 * The library is a drop-in for the reference's tc_gan/ext/libssnode.so (built
 * from tc_gan/ext/ssnode.c, bound by tc_gan/clib.py:16-33) plus an additive
 * batched ABI for the GPU-resident hot path.  Plain C: pointers and sizes
 * only, no C++/torch types.  Every entry point runs on the GPU; there is no
 * CPU fallback -- without a usable HIP device the solver symbols return
 * SSN_ERR_BASE + hipError_t (> 900, the range the reference's Python reserves
 * for "library error", tc_gan/ssnode.py:267-268).
 *
 * Conventions
 *   M = 2N neurons (E block first, then I).  W is row-major, W[i*M + j] is
 *   the weight from neuron j to neuron i (ssnode.c:64-67 `W + dim * i`).
 *   "device" pointers are hipMalloc'ed (or torch CUDA tensor) addresses on
 *   the CURRENT HIP device of the calling thread; `stream` is a hipStream_t
 *   passed as void* (NULL = the default stream).  Batched calls are
 *   asynchronous on `stream` unless stated otherwise.
 */
#ifndef SSNODE_MI355X_H
#define SSNODE_MI355X_H

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1. Drop-in symbols: exactly the exports of tc_gan/ext/ssnode.c.
 * ------------------------------------------------------------------------ */

/* Replaces ssnode.c:69-109 / 111-151 / 153-187 (ctypes decl clib.py:16-26).
 * Host fp64 buffers, caller owned: W[M*M], ext[M] read-only; r0[M] in/out;
 * r1[M] scratch.  Runs the fp64 HIP kernel (one workgroup), synchronous.
 * Returns 0 converged / 1 max_iter / 2 reached rate_hard_bound (power and
 * linear only) / >900 HIP failure.  On return the two caller buffers hold
 * what the reference's pointer-swapping loop leaves in them (newest state in
 * r0 on code 0; parity-dependent on codes 1 and 2 -- DESIGN.md "buffer
 * parity").  Re-entrant, no global mutable state beyond the HIP runtime. */
int solve_dynamics_asym_power_euler(int N, double *W, double *ext, double k, double n,
                                    double *r0, double *r1, double tau_E, double tau_I,
                                    double dt, int max_iter, double atol,
                                    double rate_soft_bound, double rate_hard_bound);
int solve_dynamics_asym_linear_euler(int N, double *W, double *ext, double k, double n,
                                     double *r0, double *r1, double tau_E, double tau_I,
                                     double dt, int max_iter, double atol,
                                     double rate_soft_bound, double rate_hard_bound);
int solve_dynamics_asym_tanh_euler(int N, double *W, double *ext, double k, double n,
                                   double *r0, double *r1, double tau_E, double tau_I,
                                   double dt, int max_iter, double atol,
                                   double rate_soft_bound, double rate_hard_bound);

/* Replace ssnode.c:21-53 (clib.py:28-33) and ssnode.c:10-19.  Scalar
 * conveniences with the reference's signatures; each call evaluates the
 * device function on the GPU for one element (see ssn_io_eval_f64 for the
 * array form).  NaN on HIP failure. */
double io_pow(double v, double r0, double r1, double v0, double k, double n);
double io_alin(double v, double r0, double r1, double v0, double k, double n);
double io_atanh(double v, double r0, double r1, double v0, double k, double n);
double rate_to_volt(double rate, double k, double n);
double dot(int dim, const double *x, const double *y);

/* ------------------------------------------------------------------------
 * 2. Additive batched ABI (new symbols).
 * ------------------------------------------------------------------------ */

#define SSN_IO_POWER  0   /* 'asym_power'  : ssnode.c io_pow   */
#define SSN_IO_LINEAR 1   /* 'asym_linear' : ssnode.c io_alin  */
#define SSN_IO_TANH   2   /* 'asym_tanh'   : ssnode.c io_atanh */
#define SSN_ERR_BASE  1000

/* Solver parameters; same meaning as the scalar arguments of the drop-in
 * symbols (ssnode.c:55-62) / tc_gan.ssnode.fixed_point (ssnode.py:159-166). */
typedef struct ssn_solver_params {
    int io_type;             /* SSN_IO_* */
    int max_iter;
    double k, n;
    double tau_E, tau_I;
    double dt;
    double atol;
    double rate_soft_bound;
    double rate_hard_bound;  /* for POWER/LINEAR: the rate_stop_at bound (ssnode.py:241-242); +inf disables */
} ssn_solver_params;

/* Library / device probes (host only). */
int         ssn_abi_version(void);
int         ssn_device_count(void);          /* <0: -hipError_t */
const char *ssn_last_error(void);            /* thread-local, "" if none */
/* Which register-resident kernel family covers a (M, NB, dtype) solve: 2 = "tile" kernel
 * (fp32: 2N <= 208, fp64: 2N <= 208), 1 = DPP kernel only, 0 = none (generic streaming
 * kernel).  The automatic dispatch of ssn_solve_batch_* additionally prefers the fp32 MFMA
 * kernels (variant 6 where it applies, else 5) for NB >= 4, 104 < 2N <= 208 and >= 192 (draw, 8 stimuli) workgroups.
 * dtype_bytes is 4 or 8. */
int         ssn_solver_fast_path(int M, int NB, int dtype_bytes);

/*
 * Batched fixed-point solve: B weight draws x NB stimuli.  Replaces the
 * thread-pool-over-ctypes loop of tc_gan/ssnode.py:423-510 for one round of
 * candidates.
 *   W      device [B][M][M]
 *   ext    device [NB][M] (ext_per_draw = 0) or [B][NB][M] (ext_per_draw = 1)
 *   r      device [B][NB][M]  in: initial rates; out: newest state
 *   r_prev device [B][NB][M] or NULL; out: state before the last executed step
 *   codes  device int32 [B][NB]: 0 / 1 / 2 as the drop-in symbols
 *   steps  device int32 [B][NB] or NULL: Euler steps executed
 * Every (draw, stimulus) pair stops independently at its own convergence /
 * bound step, exactly like an individual reference call.
 * Returns 0 or SSN_ERR_BASE + hipError_t (launch errors only; async).
 */
int ssn_solve_batch_f32(const float *W, const float *ext, int ext_per_draw,
                        float *r, float *r_prev, int *codes, int *steps,
                        int B, int NB, int M, const ssn_solver_params *p, void *stream);
int ssn_solve_batch_f64(const double *W, const double *ext, int ext_per_draw,
                        double *r, double *r_prev, int *codes, int *steps,
                        int B, int NB, int M, const ssn_solver_params *p, void *stream);
/* Force a kernel variant (testing / A-B benchmarking): 0 = generic streaming
 * kernel, 1 = register-stationary DPP kernel, 2 = register-stationary tile kernel
 * (shape chosen by the library), 3 = tile kernel with split VGPR/LDS residency where that is instantiated (what the
 * library chooses for 2 as well: the two are the same launch), 4 = tile kernel with the whole tile in VGPRs, 5 = fp32 MFMA kernel (NB >= 4), 6 = fp16-split MFMA kernel
 * (NB >= 4, asym_tanh, dt <= tau: W and the state carried as two fp16 parts each, exact products, all 8 stimuli in one
 * chain per step), 7 = the same in the alternating two-group form (state as three parts, exact), 8 = fp16-split kernel
 * with two draws per workgroup (csrc/ssn_duo.hip; what the automatic choice takes for more than 256 (draw, 8 stimuli)
 * units); error if the size has no instantiation; negative = automatic (MFMA kernel for
 * large fp32 batches with NB >= 4, otherwise tile > DPP > streaming). */
int ssn_solve_batch_f32_variant(int variant, const float *W, const float *ext, int ext_per_draw,
                                float *r, float *r_prev, int *codes, int *steps,
                                int B, int NB, int M, const ssn_solver_params *p, void *stream);
int ssn_solve_batch_f64_variant(int variant, const double *W, const double *ext, int ext_per_draw,
                                double *r, double *r_prev, int *codes, int *steps,
                                int B, int NB, int M, const ssn_solver_params *p, void *stream);

/* The variant (numbering above) that ssn_solve_batch_f32 / _f64 (dtype_bytes 4 / 8) picks by itself for this call shape
 * and these parameters under the current operand-precision setting; -1: the call would be refused.  Nothing is launched.
 * For benchmarks and logs that must name the kernel that ran. */
int ssn_solve_batch_variant_for(int B, int NB, int M, int dtype_bytes, const ssn_solver_params *p);

/* Operand precision of the AUTOMATIC kernel choice (ssn_solve_batch_* without a variant, ssn_gen_params.kernel = 0) on the
 * fp32 paths with NB >= 4 stimuli per draw.  Process-wide, atomic, takes effect with the next call; explicit variants /
 * kernel codes are never overridden.
 *   1 (initial value): the fp16-split matrix-core kernels where they apply (saturating I/O function, dt <= tau): W and the
 *      state enter the products as two fp16 parts each (23 significant bits by round to nearest in the two-draw form,
 *      22 by truncation of the state in the older wide form), every product exact, fp32 accumulation;
 *   0: fp32 operands only (fp32 MFMA / VALU kernels): the reference's floatX arithmetic.
 * The environment variable SSN_FWD_SPLIT=0 selects 0 as the initial value.  Returns the previous setting. */
int ssn_set_operand_precision(int mode);
int ssn_get_operand_precision(void);

/* Host-buffer convenience forms of the above (numpy callers): allocate,
 * copy in, solve, copy out, synchronise.  Same argument meaning, host
 * pointers.  The PCIe copies are inside the call. */
int ssn_solve_batch_host_f32(const float *W, const float *ext, int ext_per_draw,
                             float *r, float *r_prev, int *codes, int *steps,
                             int B, int NB, int M, const ssn_solver_params *p);
int ssn_solve_batch_host_f64(const double *W, const double *ext, int ext_per_draw,
                             double *r, double *r_prev, int *codes, int *steps,
                             int B, int NB, int M, const ssn_solver_params *p);

/*
 * Connectivity from noise: W[b] = make_W_with_x(z[b]; J, D, S)
 * (gradient_expressions/make_w_batch.py:8-34 == weight_gen.py:13-26).
 *   z, W   device [B][M][M];  J, D, S  HOST float/double[4] row-major 2x2
 *   (EE, EI, IE, II) -- signs applied inside (+ for E columns, - for I).
 */
int ssn_build_w_f32(const float *z, const float *J, const float *D, const float *S,
                    float *W, int B, int N, void *stream);
int ssn_build_w_f64(const double *z, const double *J, const double *D, const double *S,
                    double *W, int B, int N, void *stream);
/* ssn_build_w_f32 with J, D, S read on the DEVICE: jds_dev = device float[12] (J, D, S, each 2x2 row-major) -- e.g. the
 * parameter vector an ssn_gen_apply_f32 queued on the same stream is about to update, so that the next forward can be queued
 * before the host has read the new values.  Same arithmetic, same bits as ssn_build_w_f32 of the same values. */
int ssn_build_w_devparams_f32(const float *z, const float *jds_dev, float *W, int B, int N, void *stream);

/*
 * Stimulus: ext[b][s][pN + i] = c[b][s] * sig((x_i + bw/2)/l) * sig((bw/2 - x_i)/l),
 * x = linspace(-.5, .5, N), duplicated for E and I
 * (stimuli.py:3-10; networks/ssn.py:167-193).
 *   bandwidths, contrasts  device [B][NB];  ext device [B][NB][2N]
 */
int ssn_stimulus_f32(const float *bandwidths, const float *contrasts, float smoothness,
                     float *ext, int B, int NB, int N, void *stream);
int ssn_stimulus_f64(const double *bandwidths, const double *contrasts, double smoothness,
                     double *ext, int B, int NB, int N, void *stream);

/* ------------------------------------------------------------------------
 * 3. Fixed-time generator (BPTT path): replaces the compiled Theano graphs of
 *    tc_gan/networks/ssn.py (EulerSSNCore.get_output_for 555-576, EulerSSNModel
 *    598-633) and the reverse scan that theano.grad builds for
 *    GeneratorTrainer (networks/wgan.py:218-260).
 * ------------------------------------------------------------------------ */
typedef struct ssn_gen_params {
    int io_type;                 /* SSN_IO_* */
    int seqlen;                  /* T: Euler steps from r = 0 */
    int skip_steps;              /* first output index of the measurement window */
    int kernel;                  /* which kernels run the forward and the adjoint sweep -- the rule is DESIGN.md 3.5a:
                                  * 0 the library chooses (under ssn_set_operand_precision), 1 VALU tile / streaming
                                  * kernels; fp32 with NB >= 4 and 2N <= 208 also 2 / 3 fp32 MFMA kernels with two / one
                                  * 4-stimulus group per workgroup, and the fp16-split MFMA kernels (forward: asym_tanh
                                  * only, W as two fp16 parts; adjoint: any I/O function): 4 two groups, wide form (state
                                  * as two parts), 5 one group (state as three parts, exact), 6 two groups, alternating
                                  * form (exact state; the adjoint has one two-group form), 8 two draws per workgroup
                                  * (csrc/ssn_duo.hip, W and state as two parts by round to nearest).  Any other code is
                                  * refused. */
    double k, n;
    double tau_E, tau_I, dt;     /* eps = dt / tau per neuron */
    double rate_soft_bound, rate_hard_bound;
    double rate_penalty_threshold;
} ssn_gen_params;

/* 1 if the register-stationary generator kernels cover this size (2N <= 208 fp32, <= 104 fp64). */
int ssn_gen_supported(int M, int dtype_bytes);
/* Which fp32 forward kernel ssn_gen_forward_f32 runs for this call shape and p->kernel -- the launch's own decision, taken
 * without launching (the numbering of p->kernel; 7: wide form with an exact state, SSN_FWD_WIDE=3); seqlen replaces
 * p->seqlen; save != 0: with trajectory stores; -1: the call would be refused.  For benchmarks and tests that must name the
 * kernel they measured. */
int ssn_gen_forward_variant(int B, int NB, int M, int seqlen, int save, const ssn_gen_params *p);

/*
 * Forward: r_{t+1} = (1-eps) r_t + eps f(W r_t + ext), r_0 = 0, T = seqlen steps.
 *   W        device [B][M][M];  ext device [B][NB][M]
 *   time_avg device [B][NB][M]  mean over output indices >= skip_steps
 *   dyn_row  device [B][NB][M]  SUM over the window of (x_{t+1}-x_t)^2, per neuron -- or, from the two-draw kernel (8),
 *            per group of neurons booked on one of them (zeros elsewhere): only sum(dyn_row) is defined
 *   rate_row device [B][NB][M]  the same for relu(x_t - threshold)
 *            (dynamics_penalty = sum(dyn_row)/(B*(T-skip-1)*NB*M), rate_penalty =
 *             sum(rate_row)/(B*(T-skip)*NB*M): the means of ssn.py:626,632)
 *   traj, df device [B][NB][T][M] or both NULL: trajectory and f'(u_t) kept for the backward
 */
int ssn_gen_forward_f32(const float *W, const float *ext, float *time_avg, float *dyn_row, float *rate_row,
                        float *traj, float *df, int B, int NB, int M, const ssn_gen_params *p, void *stream);
int ssn_gen_forward_f64(const double *W, const double *ext, double *time_avg, double *dyn_row, double *rate_row,
                        double *traj, double *df, int B, int NB, int M, const ssn_gen_params *p, void *stream);
/*
 * Backward (adjoint sweep).  g_time_avg = dL/d time_avg [B][NB][M]; c_dyn, c_rate = the
 * coefficients multiplying sum(dyn_row) and sum(rate_row) in L.  `df_delta` holds the
 * forward's df on entry and delta on exit, shifted so that
 *     dL/dW[b] = df_delta[b].reshape(NB*T, M)^T @ traj[b].reshape(NB*T, M).
 */
int ssn_gen_backward_f32(const float *W, const float *traj, float *df_delta, const float *g_time_avg,
                         double c_dyn, double c_rate, int B, int NB, int M, const ssn_gen_params *p, void *stream);
int ssn_gen_backward_f64(const double *W, const double *traj, double *df_delta, const double *g_time_avg,
                         double c_dyn, double c_rate, int B, int NB, int M, const ssn_gen_params *p, void *stream);
/* Same sweep, additionally writing g_ext[B][NB][M] = dL/d ext = sum_t delta_t (gradient path of the
 * input-variability parameter V of the heterogeneous-input SSN). */
int ssn_gen_backward_ext_f32(const float *W, const float *traj, float *df_delta, const float *g_time_avg, float *g_ext,
                             double c_dyn, double c_rate, int B, int NB, int M, const ssn_gen_params *p, void *stream);
int ssn_gen_backward_ext_f64(const double *W, const double *traj, double *df_delta, const double *g_time_avg, double *g_ext,
                             double c_dyn, double c_rate, int B, int NB, int M, const ssn_gen_params *p, void *stream);
/*
 * dL/dW of the BPTT update (the `theano.grad` of networks/wgan.py:236-242 through the scan of ssn.py:354-385):
 * gW[b][i][j] = sum_k delta[b][k][i] * traj[b][k][j],  delta / traj = the [B][K = NB*T][M] views of what
 * ssn_gen_backward_* and ssn_gen_forward_* leave, gW device [B][M][M].  kernel: 0 automatic; 1 plain FMAs in k order
 * (any size, fp64); 2 (fp32, M <= 224) bf16 matrix cores on an exact three-way split of every fp32 operand, six
 * partial products per product, fp32 accumulation -- fp32 input precision at 6/16 of the fp32 MFMA cost.
 */
int ssn_weight_grad_f32(const float *delta, const float *traj, float *gW, int B, long K, int M, int kernel, void *stream);
int ssn_weight_grad_f64(const double *delta, const double *traj, double *gW, int B, long K, int M, int kernel, void *stream);
/*
 * The same product on the fp16 matrix cores: every operand as two fp16 numbers by round to nearest (x 2^e = h + m to 2^-24),
 * three partial products per product, fp32 accumulation -- the accuracy of kernel 2 at half its matrix work.  fp16 has five
 * exponent bits, so the caller supplies bounds: dmax device [B], dmax[b] >= max |delta[b]| (one power-of-two scale per
 * draw; elements below 2^-40 of it are lost), and xmax >= max |traj| (host scalar, > 0 and finite: the rate bound of the
 * saturating I/O function).  A bound that is too small overflows fp16: inf / NaN in gW, never a silently wrong value.
 * ssn_gen_backward_max_f32 is ssn_gen_backward_ext_f32 plus that bound: when the sweep that runs tracks max |delta| per draw
 * (the fp16-split kernels 4 / 5 / 6 / 8, which need it for their own scaling) it fills dmax[B] and sets *tracked = 1; otherwise *tracked = 0,
 * dmax is untouched and ssn_weight_grad_f32 is the kernel to call.  fp32, M <= 224.
 */
/*
 * The adjoint sweep and dL/dW in ONE launch (the two halves of the same `theano.grad`, networks/wgan.py:236-242 through
 * ssn.py:354-385): what ssn_gen_backward_max_f32 followed by ssn_weight_grad_scaled_f32 compute, without the delta
 * stream between them -- a draw's dL/dW accumulates in the register file of the workgroup that runs its sweep.
 * df [B][NB][T][M] (f'(u) of the forward) is only read; gW device [B][M][M]; g_ext [B][NB][M] or NULL; dmax device [B]
 * or NULL (max |delta| per draw; NaN marks a draw whose delta outgrew its lagged fp16 scale, and its gW is NaN too);
 * xmax >= max |traj| as for ssn_weight_grad_scaled_f32.  fp32, NB <= 8, even 2N <= 208: ..._supported answers 1 / 0 for a
 * shape, and the entry refuses the others (no fallback inside).
 */
int ssn_gen_backward_fused_supported(int B, int NB, int M, const ssn_gen_params *p, float xmax);
int ssn_gen_backward_fused_f32(const float *W, const float *traj, const float *df, const float *g_time_avg, float *g_ext,
                               float *gW, float *dmax, float xmax, double c_dyn, double c_rate, int B, int NB, int M,
                               const ssn_gen_params *p, void *stream);
int ssn_gen_backward_max_f32(const float *W, const float *traj, float *df_delta, const float *g_time_avg, float *g_ext,
                             float *dmax, int *tracked, double c_dyn, double c_rate, int B, int NB, int M,
                             const ssn_gen_params *p, void *stream);
int ssn_weight_grad_scaled_f32(const float *delta, const float *traj, float *gW, int B, long K, int M, const float *dmax,
                               float xmax, void *stream);
/*
 * Chain rule W -> (J, D, S) of make_W_with_x (make_w_batch.py:19-34): out[b][pq][0..2] =
 * partial dL/dJ_pq, dL/dD_pq, dL/dS_pq of draw b (device fp64 [B][4][3]; sum over b on the caller's
 * side in a fixed order).  J, D, S are HOST arrays of 4.
 */
int ssn_jds_grad_f32(const float *gW, const float *z, const float *J, const float *D, const float *S,
                     double *out, int B, int N, void *stream);
int ssn_jds_grad_f64(const double *gW, const double *z, const double *J, const double *D, const double *S,
                     double *out, int B, int N, void *stream);

/* ------------------------------------------------------------------------
 * 4. WGAN-GP critic and optimizers: replace the compiled Theano graphs of
 *    ConditionalDiscriminator / ConditionalCriticTrainer (networks/cwgan.py:123-214),
 *    the critic part of GeneratorTrainer's loss (networks/wgan.py:236) and
 *    Updater (networks/wgan.py:111-165 over lasagne.updates.*).
 *    Network: h0 = [x(nx), contrast, |norm_probe|, cell_type]; L hidden ReLU layers
 *    (normalization 'none'); linear 1-unit output without bias.
 *    params / grads: ONE flat fp32 device buffer [W_1 (n0 x n1) row-major, b_1, ...,
 *    W_L, b_L, w_out (n_L)] -- the order of lasagne.layers.get_all_params.
 *    dims: HOST int[L+1] = {n0 = nx+3, n1, ..., nL}.
 *    Unconditional critic (UnConditionalDiscriminator, networks/wgan.py:66-97; CriticTrainer,
 *    wgan.py:194-215): pass NULL for EVERY condition pointer of a call (cond; cg, cd and cp
 *    together) -- then h0 = x and dims[0] = nx.  Conditions for some inputs of a call and not
 *    for others are refused.
 *    precision: 0 = bf16 MFMA operands (fp32 accumulate), 1 = fp32 MFMA.
 * ------------------------------------------------------------------------ */
long   ssn_critic_num_params(const int *dims, int nlayers);
size_t ssn_critic_workspace_floats(const int *dims, int nlayers, int batch_gd, int batch_p);
/* out[batch] = D(x, cond).  x device [batch][nx], cond device [batch][3] (contrast, norm_probe, cell_type). */
int ssn_critic_forward(const float *params, const int *dims, int nlayers, const float *x, const float *cond,
                       int batch, int hide_cell_type, float *out, float *workspace, int precision, void *stream);
/* loss = mean D(xg) - mean D(xd) + lmd * mean((||dD/dxp|| - 1)^2) and d loss / d params.
 * stats device float[4] = {mean D(xg), mean D(xd), penalty, loss}; dvals device [ng+nd] = D of [xg; xd]. */
int ssn_critic_loss_grad(const float *params, const int *dims, int nlayers,
                         const float *xg, const float *cg, const float *xd, const float *cd,
                         const float *xp, const float *cp, int ng, int nd, int np, float lmd,
                         int hide_cell_type, float *grads, float *stats, float *dvals,
                         float *workspace, int precision, void *stream);
/* gx[batch][nx] = scale * d(mean-free sum_b D_b)/dx, stats[0] = mean D(x)  (generator side: scale = -1/batch). */
int ssn_critic_input_grad(const float *params, const int *dims, int nlayers, const float *x, const float *cond,
                          int batch, int hide_cell_type, float scale, float *gx, float *stats,
                          float *workspace, int precision, void *stream);

/* The same three passes with the hidden nonlinearity x > 0 ? x : leak * x, 0 <= leak <= 1: lasagne's `rectify` (0),
 * `leaky_rectify` (0.01), `very_leaky_rectify` (1/3), `linear` / `identity` (1) -- the piecewise-linear choices of
 * simple_discriminator.py:139-152, for which the input gradient stays a linear chain with fixed slopes and the WGAN-GP double
 * backward keeps its form.  Plain (not layer-normalised) layers, layer-by-layer path. */
int ssn_critic_forward_leaky(const float *params, const int *dims, int nlayers, const float *x, const float *cond,
                             int batch, int hide_cell_type, float leak, float *out, float *workspace, int precision,
                             void *stream);
int ssn_critic_loss_grad_leaky(const float *params, const int *dims, int nlayers,
                               const float *xg, const float *cg, const float *xd, const float *cd,
                               const float *xp, const float *cp, int ng, int nd, int np, float lmd,
                               int hide_cell_type, float leak, float *grads, float *stats, float *dvals,
                               float *workspace, int precision, void *stream);
int ssn_critic_input_grad_leaky(const float *params, const int *dims, int nlayers, const float *x, const float *cond,
                                int batch, int hide_cell_type, float leak, float scale, float *gx, float *stats,
                                float *workspace, int precision, void *stream);

/* acc[0] = mean D(xg) - mean D(xd) (the "accuracy" of cwgan.py:139-147, logged after every critic update) in one call: two
 * forwards into dvals (device [ng + nd], scratch), one reduction in a fixed order.  layer_norm: HOST int[L] or NULL; leak as
 * above; workspace as for ssn_critic_forward* with batch = max(ng, nd). */
int ssn_critic_accuracy(const float *params, const int *dims, const int *layer_norm, int nlayers, float leak,
                        const float *xg, const float *cg, const float *xd, const float *cd, int ng, int nd,
                        int hide_cell_type, float *acc, float *dvals, float *workspace, int precision, void *stream);

/* The same three passes for a critic whose hidden layer l is layer-normalised when layer_norm[l] != 0
 * (simple_discriminator.py:51-75: Dense(no bias) -> LayerNorm (eps 1e-4, no parameters) -> Bias -> ReLU;
 * same [W_l, b_l] parameter layout).  layer_norm: HOST int[L] or NULL (all plain).  The WGAN-GP double
 * backward goes through the normalisation. */
size_t ssn_critic_norm_workspace_floats(const int *dims, int nlayers, int batch_gd, int batch_p);
int ssn_critic_forward_norm(const float *params, const int *dims, const int *layer_norm, int nlayers,
                            const float *x, const float *cond, int batch, int hide_cell_type, float *out,
                            float *workspace, int precision, void *stream);
int ssn_critic_loss_grad_norm(const float *params, const int *dims, const int *layer_norm, int nlayers,
                              const float *xg, const float *cg, const float *xd, const float *cd,
                              const float *xp, const float *cp, int ng, int nd, int np, float lmd,
                              int hide_cell_type, float *grads, float *stats, float *dvals,
                              float *workspace, int precision, void *stream);
int ssn_critic_input_grad_norm(const float *params, const int *dims, const int *layer_norm, int nlayers,
                               const float *x, const float *cond, int batch, int hide_cell_type, float scale,
                               float *gx, float *stats, float *workspace, int precision, void *stream);

/* The same passes for any critic, up to its general form (simple_discriminator.py:57-75, 139-152; `--disc-nonlinearity`,
 * run/bptt_wgan.py:153): hidden nonlinearity act = 0 rectify, 1 leaky_rectify (0.01), 2 very_leaky_rectify (1/3), 3 linear,
 * 4 tanh, 5 sigmoid, 6 softplus, 7 elu (lasagne.nonlinearities); layer_flags: HOST int[L] or NULL, per hidden layer 0 = plain
 * Dense + bias, 1 = Dense(no bias) -> LayerNorm -> Bias, 3 = Dense(no bias) -> LayerNorm -> ScaleLayer -> Bias (the reference
 * inserts the learnable per-unit scale for every nonlinearity but rectify).  Parameter layout per layer: W [in][out],
 * scales [out] (flag 3 only), b [out]; then w_out -- lasagne's get_all_params order.  The gradient penalty's double backward
 * carries the curvature f'' of the smooth nonlinearities and the scales' gradients.
 * These calls describe the critic; the library chooses the fastest kernels that compute it, so a critic that
 * one of the families above also describes runs exactly as it does there.  Workspace: ssn_critic_norm_workspace_floats
 * (enough for every path); ssn_critic_workspace_floats is enough for a piecewise-linear critic (act 0-3) without normalisation. */
long ssn_critic_num_params_act(const int *dims, const int *layer_flags, int nlayers);
int ssn_critic_forward_act(const float *params, const int *dims, const int *layer_flags, int nlayers, int act,
                           const float *x, const float *cond, int batch, int hide_cell_type, float *out,
                           float *workspace, int precision, void *stream);
int ssn_critic_loss_grad_act(const float *params, const int *dims, const int *layer_flags, int nlayers, int act,
                             const float *xg, const float *cg, const float *xd, const float *cd,
                             const float *xp, const float *cp, int ng, int nd, int np, float lmd,
                             int hide_cell_type, float *grads, float *stats, float *dvals,
                             float *workspace, int precision, void *stream);
int ssn_critic_input_grad_act(const float *params, const int *dims, const int *layer_flags, int nlayers, int act,
                              const float *x, const float *cond, int batch, int hide_cell_type, float scale,
                              float *gx, float *stats, float *workspace, int precision, void *stream);
int ssn_critic_accuracy_act(const float *params, const int *dims, const int *layer_flags, int nlayers, int act,
                            const float *xg, const float *cg, const float *xd, const float *cd, int ng, int nd,
                            int hide_cell_type, float *acc, float *dvals, float *workspace, int precision, void *stream);

typedef struct ssn_opt_params {
    int kind;                 /* 0 sgd, 1 adam, 2 rmsprop (lasagne.updates) */
    int step;                 /* 1-based update count (adam bias correction) */
    int clip;                 /* clamp the new value to [clip_lo, clip_hi] (wgan.py:244-251) */
    int reserved;             /* bit 0 (ssn_gen_apply_f32 with a record, n <= 64): make NO update when any gradient element is not
                               * finite -- parameters and optimizer state stay, record = the old values, record[n] = NaN */
    double learning_rate, beta1, beta2, epsilon, rho;
    double reg_l2_penalty, reg_l1_penalty, reg_l2_decay, reg_l1_decay;   /* wgan.py:121-129 */
    double clip_lo, clip_hi;
} ssn_opt_params;
/* In-place update of p[n] from g[n]; s1, s2 optimizer state (adam: m, v; rmsprop: s1 only; sgd: unused). */
int ssn_optimizer_step(float *p, const float *g, float *s1, float *s2, long n, const ssn_opt_params *o, void *stream);

/*
 * One critic step of the GAN loop in ONE call (single process; the data-parallel loop keeps the separate calls because its
 * all-reduce sits between the gradient and the optimizer step): penalty points xp = eps xd + (1 - eps) xg (cwgan.py:476-481),
 * loss + gradient (ssn_critic_loss_grad*), optimizer step on the critic's parameters, accuracy of the UPDATED critic
 * (cwgan.py:507), per-tensor sums of squares of the updated parameters (recorders.py:275-311), and the step's scalar record
 * tail[4 + nseg] = {dynamics penalty, rate penalty (from pens64, device double[2] or NULL), loss, accuracy, sums of squares}.
 * The same kernels in the same order as the separate calls: identical results.  xg, xd: device [n][nx]; cond [n][3] shared by
 * the three inputs; eps device [n]; layer_norm / leak as above; opt_s1 / opt_s2 / opt as ssn_optimizer_step; seg_bounds, seg_ws
 * as ssn_segment_sqnorms2_f32; acc_dvals device [2 n] scratch; workspace as ssn_critic_*workspace_floats(n + n, n).
 */
typedef struct ssn_critic_step {
    float *params; const int *dims; const int *layer_norm; int nlayers; float leak;
    const float *xg, *xd, *cond, *eps;
    int n, hide_cell_type, precision; float lmd;
    float *xp, *grads, *stats, *dvals, *workspace;
    float *opt_s1, *opt_s2; const ssn_opt_params *opt;
    const long *seg_bounds; int nseg; double *seg_ws;
    const double *pens64;
    float *acc_dvals, *tail;
} ssn_critic_step;
int ssn_critic_step_run(const ssn_critic_step *a, void *stream);
/* The same with the rule of cwgan.py:493-498 decided on the device: the optimizer step (parameters AND optimizer state) is
 * skipped when the batch's rate penalty pens64[1] exceeds rate_penalty_bound (> 0; pens64 required).  Everything else runs and
 * is written as in ssn_critic_step_run -- the caller reads tail[1], sees the bound exceeded and reports the step as skipped
 * (loss and accuracy NaN in the reference's record); no host round trip, no snapshot to roll back to. */
int ssn_critic_step_gated_run(const ssn_critic_step *a, double rate_penalty_bound, void *stream);

/*
 * End of a generator step (GeneratorTrainer, networks/wgan.py:218-260) in two calls, with the job's all-reduce (if any)
 * between them.  ssn_gen_grads_f32, ONE launch: out[nv + 12 + 1] = {dL/dV (nv = 0: none; 1: 'deg-heteroin', one V for both
 * populations; 2: 'heteroin', V_E, V_I), dL/dJ[4], dL/dD[4], dL/dS[4], loss} from jds_part (device [B][4][3], the output of
 * ssn_jds_grad_*), the input-variability pieces g_ext, ext_base (device [B][NB][M]) and zin (device [B][M]) --
 * dL/dV_pop = sum over draws, stimuli and the population's neurons of g_ext ext_base zin (networks/ssn.py:679-686) --
 * and loss = -dmean[0] + dynamics_cost pens64[0] + rate_cost pens64[1] (wgan.py:236-241; dmean: mean D(G(z)), stats[0] of
 * ssn_critic_input_grad*; pens64 may be NULL = 0).  Sums in fp64, fixed order.  ws: device scratch of
 * ssn_gen_grads_ws_doubles() doubles whose LAST 8 bytes are zero before the first call (the kernel leaves them zero).
 * ssn_gen_apply_f32, ONE launch: the update of ssn_optimizer_step on all n parameters at once with per-element clip bounds
 * clip_lo / clip_hi (device [n]; both NULL = opt's scalar rule) -- the reference clips with numpy broadcasting,
 * wgan.py:244-251 -- and record[n + 1] (device, or NULL) = the new values followed by grads[n] (the loss riding behind the
 * gradient vector).
 */
typedef struct ssn_gen_grads {
    const double *jds_part; int B;
    int nv;
    const float *g_ext, *ext_base, *zin; int NB, M;
    const float *dmean; const double *pens64;
    double dynamics_cost, rate_cost;
    double *ws;
    float *out;
} ssn_gen_grads;
long ssn_gen_grads_ws_doubles(void);
int ssn_gen_grads_f32(const ssn_gen_grads *a, void *stream);
int ssn_gen_apply_f32(float *params, const float *grads, float *s1, float *s2, int n, const ssn_opt_params *opt,
                      const float *clip_lo, const float *clip_hi, float *record, void *stream);

/* ------------------------------------------------------------------------
 * 5. Feed-forward tuning-curve generator (FF_lalazar model; BASELINE config 5): replaces the Theano
 *    graph of FF_functions/lalazar_func.py:16-45 (get_FF_output) compiled at
 *    FF_lalazar_model.py:175-179.  Grid = box^3 points of linspace(-3, 3, box)^3, z fastest.
 * ------------------------------------------------------------------------ */
typedef struct ssn_ff_params {
    int nsam, nhid, ni, box;
    double RF_l, RF_d, TH, TH_d, J, a;   /* already exponentiated where the model script does (FF_lalazar_model.py:175) */
} ssn_ff_params;
/* out[nsam][ni][nhid] = relu(sum_g e w / sum_g e - thr).  RF_w [nsam][G], FF_con/FF_str [nsam][nhid][G],
 * TH_sam [nsam][nhid], stim [ni][3] (ni <= 32), all device fp32.  q, den [nsam][ni][nhid] optional (NULL):
 * pre-threshold drive and sum_g e, kept for the backward.  When box^3 % 4 == 0 the kernels read RF_w, FF_con and FF_str with
 * 16-byte loads: the three pointers must then be 16-byte aligned, and the call is refused with the invalid-argument status
 * (nothing is launched) when one is not.  The connection-list entry points below take any 4-byte aligned pointers. */
int ssn_ff_forward_f32(const float *RF_w, const float *FF_con, const float *FF_str, const float *TH_sam,
                       const float *stim, float *out, float *q, float *den, const ssn_ff_params *p, void *stream);
/* The same outputs from the model's own data structure: a unit has box^3 / 100 connections (FF_lalazar_model.py:154-167), so
 * instead of the dense FF_con / FF_str streams (99 % zeros, 8 of the 12 bytes per point) the connections come as lists:
 * conn_idx[nsam][nhid][ncon] (device int32, grid index z fastest, each index at most once per unit; < 0 = empty slot) and
 * conn_str[nsam][nhid][ncon] (the strengths FF_str at those indices).  sum_g e runs over all points of RF_w (4 B per point,
 * shared by the sample's hidden units), sum_g e w over the list. */
int ssn_ff_forward_sparse_f32(const float *RF_w, const int *conn_idx, const float *conn_str, int ncon, const float *TH_sam,
                              const float *stim, float *out, float *q, float *den, const ssn_ff_params *p, void *stream);
/* ssn_ff_backward_f32 (below) from the same lists: dsig as there. */
int ssn_ff_backward_sparse_f32(const float *RF_w, const int *conn_idx, const float *conn_str, int ncon, const float *stim,
                               const float *q, const float *den, const float *gq, float *dsig, const ssn_ff_params *p,
                               void *stream);
/* dsig[nsam][nhid][2] = per-sample partial derivatives of L w.r.t. RF_l and RF_d, given gq[nsam][ni][nhid] =
 * dL/d(drive) (upstream gradient times [out > 0]) and the forward's q, den.  RF_w, FF_con, FF_str: the alignment contract of
 * ssn_ff_forward_f32 (16-byte aligned when box^3 % 4 == 0, refused otherwise). */
int ssn_ff_backward_f32(const float *RF_w, const float *FF_con, const float *FF_str, const float *stim,
                        const float *q, const float *den, const float *gq, float *dsig,
                        const ssn_ff_params *p, void *stream);

/* ---- 6. Moment matching (tc_gan/networks/moment_matching.py:91-104, 221-243; run/bptt_moments.py) ------------
 * x[B][D] generated tuning curves (device fp32).  sums[2][D] (device fp64) = (sum_b x, sum_b x^2): all-reduce it
 * over ranks when the minibatch is sharded, then pass the GLOBAL batch size.  data_moments, weights: [2][D] device
 * fp64 (BPTTMomentMatcher.set_dataset).  gx[B][D] = d L0 / d x with L0 = mean(weights * (data_moments - (m, s))^2);
 * out[1 + 2 D] (device fp64) = L0, m[D], s[D]  (sample mean / population variance of the minibatch). */
int ssn_moment_sums_f32(const float *x, int B, int D, double *sums, void *stream);
int ssn_moment_loss_grad_f32(const float *x, const double *sums, double global_batch, const double *data_moments,
                             const double *weights, int B, int D, float *gx, double *out, void *stream);

/* ---- 6b. Ensembles of moment-matching runs (networks/moment_matching_ensemble.py) -------------------------------------
 * K independent runs share the generator launches of a step: member k owns the contiguous draws [k B, (k + 1) B) of every
 * batch (x[K B][D], W[K B][2N][2N], ...).  Per-member values come in small device arrays indexed by the member.  Each call is
 * ONE launch whatever K is (ssn_ens_moments_f32: two), and every sum of a member runs over its own rows: a non-finite value in
 * one member reaches no other member.  The record: one fp64 row of ssn_ens_record_doubles(D, P) doubles per member, row
 * stride rstride >= that --
 *   [0] L0, [1 .. D] m, [1 + D .. 2D] s, [1 + 2D] dynamics_penalty, [2 + 2D] rate_penalty (both rounded to fp32), [3 + 2D] loss,
 *   [4 + 2D .. 4 + 2D + P) the new parameters, then the P gradients (P = nv + 12) --
 * the one buffer the host reads back per step.
 * ssn_ens_moments_f32: ssn_moment_sums_f32 + ssn_moment_loss_grad_f32 per member with the member's batch B (the same loops:
 *   the same bits as the single run); sums: device [K][2][D] scratch; data_moments, weights: device [K][2][D]; m and s go to
 *   the record, L0 is formed by ssn_ens_gen_grads_f32.
 * ssn_ens_jds_grad_f32: ssn_jds_grad_f32 per member; p16: device [K][16] fp32 = J[4], D[4], 1 / (2 S^2)[4], 1 / S^3[4] (each S
 *   term rounded as launch_jds_grad rounds it: 1.f / ((2.f * s) * s), 1.f / ((s * s) * s)); out: device [K B][4][3].
 * ssn_ens_gen_grads_f32: grads[K][nv + 12] = ssn_gen_grads_f32's dL/dV, dL/dJ, dL/dD, dL/dS per member; the penalty means of the
 *   forward's rows dyn_row / rate_row over the member's draws (scale_*: 1 / element count of ONE member); L0 and
 *   loss = L0 + costs[k][0] dyn + costs[k][1] rate into the record.  One workgroup per member, fp64 sums in a fixed order.
 *   D >= 1 (L0 is a mean over the 2 D moments); D = 0 is refused: a loss without moments takes ssn_ens_gen_grads_l0_f32.
 * ssn_ens_apply_f32: ssn_optimizer_step's update of all K parameter vectors p[K][P] (states s1, s2 [K][P]) with
 *   hyp[k][8] = (learning_rate, a_t, reg_l2_penalty, reg_l1_penalty, reg_l2_decay, reg_l1_decay, -, -) per member (a_t: Adam's
 *   lr sqrt(1 - beta2^t) / (1 - beta1^t), formed by the caller) and per-element clip bounds [K][P]; a NaN value stays NaN.
 * ssn_ens_stimulus_hetero_f32: ssn_stimulus_hetero_f32 (nv = 2) with v[k][2] = (V_E, V_I) of the draw's member. */
typedef struct ssn_ens_grads {
    int K, B, nv, NB, M, D;
    const double *part;
    const float *g_ext, *ext_base, *zin;
    const float *dyn_row, *rate_row;
    double scale_dyn, scale_rate;
    const double *data_moments, *weights, *costs;
    float *grads;
    double *rec; int rstride;
} ssn_ens_grads;
typedef struct ssn_ens_apply {
    int K, P, kind;
    float beta1, beta2, eps, rho;
    const float *hyp;
    const float *clip_lo, *clip_hi;
    float *p, *s1, *s2; const float *g;
    double *rec; int rstride, rec_off;
} ssn_ens_apply;
long ssn_ens_record_doubles(int D, int P);
int ssn_ens_moments_f32(const float *x, int K, int B, int D, double *sums, const double *data_moments, const double *weights,
                        float *gx, double *rec, int rstride, void *stream);
int ssn_ens_jds_grad_f32(const float *gW, const float *z, const float *p16, double *out, int K, int B, int N, void *stream);
int ssn_ens_gen_grads_f32(const ssn_ens_grads *a, void *stream);
int ssn_ens_apply_f32(const ssn_ens_apply *a, void *stream);
int ssn_ens_stimulus_hetero_f32(const float *bw, const float *con, float smoothness, const float *zin, const float *v, float *ext,
                                int K, int B, int NB, int N, void *stream);

/* ---- 7. Fixed-point implicit gradient (tc_gan/gradient_expressions/SS_grad.py:17-99, make_w_batch.py:36-121) -----
 * dW[b][i][j][p][q] = d W[b][i][j] / d theta[p][q] for theta = J (which 0; independent of z, z may be NULL),
 * D (1) or S (2): the tensors make_WJ_with_x / make_WD_with_x / make_WS_with_x build (identity dJ'/dJ). */
int ssn_build_dw_f32(const float *z, const float *J, const float *D, const float *S, int which, float *dW, int B, int N,
                     void *stream);
int ssn_build_dw_f64(const double *z, const double *J, const double *D, const double *S, int which, double *dW, int B,
                     int N, void *stream);
/* The batched linear systems of WRgrad_batch at fixed points R[nz][nb][M]:  A[z][b] = 1 - Phi W[z],
 * rhs[z][b][i][c] = Phi_i * sum_j dW[z][i][j][c] R[z][b][j],  Phi = f'(W R + I) (I [nb][M], or [nz][nb][M] when
 * i_per_draw; dW [nz][M][M][4], or [1][M][M][4] when !dw_per_draw).  Solving A x = rhs gives dR/dtheta[z][b][M][2][2].
 * p: io_type, k, n, rate_soft_bound, rate_hard_bound are used.  All device pointers. */
int ssn_ss_grad_system_f32(const float *R, const float *W, const float *dW, int dw_per_draw, const float *I,
                           int i_per_draw, int nz, int nb, int M, const ssn_solver_params *p, float *A, float *rhs,
                           void *stream);
int ssn_ss_grad_system_f64(const double *R, const double *W, const double *dW, int dw_per_draw, const double *I,
                           int i_per_draw, int nz, int nb, int M, const ssn_solver_params *p, double *A, double *rhs,
                           void *stream);

/* Heterogeneous-input variant (networks/ssn.py:645-772): ext *= amp[b][m], amp = 1 + v_pop * z_in,
 * device [B][2N] (NULL = homogeneous). */
int ssn_stimulus_amp_f32(const float *bandwidths, const float *contrasts, float smoothness, const float *amp,
                         float *ext, int B, int NB, int N, void *stream);
int ssn_stimulus_amp_f64(const double *bandwidths, const double *contrasts, double smoothness, const double *amp,
                         double *ext, int B, int NB, int N, void *stream);
/* The same with the amplification formed in the launch (networks/ssn.py:679-686): amp[b][m] = 1 + v(m) * zin[b][m], rounded as
 * the two fp32 operations of `1 + vs[None, :] * zin`.  zin: device [B][2N]; v: device, one value per neuron (nv = 2N), per
 * population (nv = 2: neurons 0..N-1 take v[0], the others v[1]) or one for all (nv = 1). */
int ssn_stimulus_hetero_f32(const float *bandwidths, const float *contrasts, float smoothness, const float *zin, const float *v,
                            int nv, float *ext, int B, int NB, int N, void *stream);

/* I/O nonlinearity on arrays (device pointers), the device function the solver
 * kernels use: out[i] = io(v[i]).  p->k, n, rate_soft_bound, rate_hard_bound,
 * io_type are read; for SSN_IO_* semantics see ssnode.c:25-53. */
int ssn_io_eval_f32(const float *v, float *out, long count, const ssn_solver_params *p, void *stream);
int ssn_io_eval_f64(const double *v, double *out, long count, const ssn_solver_params *p, void *stream);

/* Batched dense solve for the implicit gradient (the `solve` of tc_gan/gradient_expressions/SS_grad.py:44, once per
 * (draw, stimulus)): A [nsys][M][M] row-major and rhs [nsys][M][nrhs] (nrhs = 4 or 1), device pointers, both
 * OVERWRITTEN -- A with its LU factors (partial row pivoting), rhs with the solution.  info (device, [nsys], may be
 * NULL): 0, or 1 + the first elimination step whose pivot column was all zero. */
int ssn_lu_solve_f32(float *A, float *rhs, int *info, int nsys, int M, int nrhs, void *stream);
int ssn_lu_solve_f64(double *A, double *rhs, int *info, int nsys, int M, int nrhs, void *stream);

/* The two scalar penalties of the fixed-time generator from the per-neuron window sums ssn_gen_forward_* leaves
 * (networks/ssn.py:626, 632): out[0] = scale_dyn * sum(dyn_row), out[1] = scale_rate * sum(rate_row), fp64, one launch,
 * deterministic.  ws: device scratch of 2 * 256 + 1 doubles whose LAST 8 bytes are zero before the first call (the
 * kernel leaves them zero); out: device [2]. */
int ssn_penalty_means_f32(const float *dyn_row, const float *rate_row, long n, double scale_dyn, double scale_rate,
                          double *ws, double *out, void *stream);
int ssn_penalty_means_f64(const double *dyn_row, const double *rate_row, long n, double scale_dyn, double scale_rate,
                          double *ws, double *out, void *stream);
/* The same launch with the conditional prober's gather riding along (cwgan.py:91-98; one launch instead of two):
 * tc[k][s] = time_avg[ids[k]][s][probes[k]] for k < nsamp, s < NB (time_avg: device [B][NB][M]; ids, probes: device int64
 * [nsamp], 0 <= ids < B, 0 <= probes < M; tc: device [nsamp][NB]).  nsamp = 0: exactly ssn_penalty_means_*. */
int ssn_penalty_means_probe_f32(const float *dyn_row, const float *rate_row, long n, double scale_dyn, double scale_rate,
                                double *ws, double *out, const float *time_avg, const long *ids, const long *probes,
                                float *tc, int nsamp, int NB, int M, void *stream);
int ssn_penalty_means_probe_f64(const double *dyn_row, const double *rate_row, long n, double scale_dyn, double scale_rate,
                                double *ws, double *out, const double *time_avg, const long *ids, const long *probes,
                                double *tc, int nsamp, int NB, int M, void *stream);
/* Per-step helpers of the GAN loop.  ssn_segment_sqnorms2_f32: out[t] = sum of x[i]^2 over
 * bounds[t] <= i < bounds[t + 1] (the per-tensor critic statistics of recorders.py:275-311; bounds: device [n + 1], out:
 * device [n]; ws: device scratch of ssn_segment_sqnorms_ws_doubles(n) doubles; every tensor is cut into chunks summed by
 * their own workgroups in fp64, the chunk sums added in chunk order: the same bits every run).
 * ssn_segment_sqnorms_f32 keeps the signature this symbol had before the scratch argument existed (same results; the
 * scratch comes from the stream-ordered allocator): a caller built against the older header still links AND runs right.
 * ssn_interpolate_f32: xp[r][c] = eps[r] xd[r][c] + (1 - eps[r]) xg[r][c], the
 * gradient-penalty points of cwgan.py:476-481 (all device; xd, xg, xp [rows][cols], eps [rows]). */
long ssn_segment_sqnorms_ws_doubles(int n);
int ssn_segment_sqnorms2_f32(const float *x, const long *bounds, int n, float *out, double *ws, void *stream);
int ssn_segment_sqnorms_f32(const float *x, const long *bounds, int n, float *out, void *stream);
/* Adjoint of the conditional prober's gather tuning_curve[k][s] = time_avg[ids[k]][s][probes[k]] (cwgan.py:91-98):
 * g_ta[b][s][m] = sum of g[k][s] over the samples k with ids[k] == b, probes[k] == m; the whole of g_ta is written.
 * g: device [n][NB], ids / probes: device int64 [n] (0 <= ids < B, 0 <= probes < M), g_ta: device [B][NB][M].
 * Samples are added in k order: deterministic. */
int ssn_probe_scatter_f32(const float *g, const long *ids, const long *probes, float *g_ta, int n, int B, int NB, int M, void *stream);
int ssn_probe_scatter_f64(const double *g, const long *ids, const long *probes, double *g_ta, int n, int B, int NB, int M, void *stream);
int ssn_interpolate_f32(const float *eps, const float *xd, const float *xg, float *xp, int rows, int cols, void *stream);

/* Device-side noise for the generator's z (replaces the host `rng.rand(batch, 2N, 2N)` of
 * tc_gan/networks/ssn.py:434-439 in the opt-in performance mode; the reference has no such mode, parity runs keep
 * host noise).  out[i] = u(seed, offset + i) in [0, 1) with 24 random bits, from Philox4x32-10 (Salmon, Moraes,
 * Dror, Shaw, SC'11; known-answer vectors checked in tests/test_noise.py): element g of the stream is word g % 4 of
 * the block with counter (g / 4, 0, 0, 0) and key (seed lo, seed hi).  Any slice can be generated by itself, so the
 * ranks of a data-parallel job each fill their own rows of ONE global stream.  `out` is a device pointer. */
int ssn_philox_uniform_f32(unsigned long long seed, unsigned long long offset, float *out, unsigned long long n, void *stream);
int ssn_philox_uniform_f64(unsigned long long seed, unsigned long long offset, double *out, unsigned long long n, void *stream);
/*
 * ssn_philox_uniform_* followed by ssn_build_w_* in one launch: W[b] = make_W_with_x(z[b]; J, D, S) with z = the B*M*M
 * stream elements from `offset` on (bit for bit the numbers ssn_philox_uniform_* writes).  z: device [B][M][M] to keep the
 * draw (the generator update's chain rule reads it), or NULL -- then the noise never touches memory.  W (and z) must be
 * 16-byte aligned; otherwise invalid-argument, and the two calls above are the path.
 */
int ssn_build_w_philox_f32(unsigned long long seed, unsigned long long offset, const float *J, const float *D, const float *S,
                           float *W, float *z, int B, int N, void *stream);
int ssn_build_w_philox_f64(unsigned long long seed, unsigned long long offset, const double *J, const double *D, const double *S,
                           double *W, double *z, int B, int N, void *stream);
/*
 * Everything a device-noise generator forward reads, in ONE call (the launches of ssn_philox_amp_f32, ssn_stimulus_amp_f32 and
 * ssn_build_w_philox_f32 in that order: the same numbers, without the host between them): zin / amp = the heterogeneous-input
 * signs and 1 + v zin from stream elements off_zin.. (v device [M]; v NULL: none, plain stimulus), ext[B][NB][M] the (amplified)
 * stimulus of bandwidths bw and contrasts con (device [B][NB]), W[B][M][M] from stream elements off_z.. (z device or NULL).
 * amp, and the gain inside ext, are 1 + v zin as TWO fp32 operations (the product is rounded, then the sum: the bits of
 * ssn_stimulus_hetero_f32 and of the torch expression `1 + vs[None, :] * zin`), so ext equals ssn_stimulus_amp_f32 of the
 * returned amp and ssn_stimulus_hetero_f32 of the returned zin bit for bit (tests/test_device_inputs_gpu.py).
 */
typedef struct ssn_gen_inputs {
    unsigned long long seed, off_z, off_zin;
    const float *J, *D, *S;            /* HOST float[4] each */
    const float *bw, *con;
    float smoothness;
    const float *v;
    int bernoulli;
    float *W, *z, *zin, *amp, *ext;
    int B, NB, N;
} ssn_gen_inputs;
int ssn_gen_inputs_philox_f32(const ssn_gen_inputs *a, void *stream);
/* The heterogeneous-input SSN's noise from the same stream, in one launch (networks/ssn.py:679-720): zin[i] = +1 / -1
 * (u < 0.5; bernoulli != 0) or 2 u - 1, and amp[i] = 1 + v[i % M] * zin[i] (v: device [M], the input variability per
 * neuron; two operations of the type: the product is rounded before the sum); zin, amp: device [n]. */
int ssn_philox_amp_f32(unsigned long long seed, unsigned long long offset, const float *v, float *zin, float *amp,
                       unsigned long long n, int M, int bernoulli, void *stream);
int ssn_philox_amp_f64(unsigned long long seed, unsigned long long offset, const double *v, double *zin, double *amp,
                       unsigned long long n, int M, int bernoulli, void *stream);

/*
 * The reference's OWN noise stream on the device: numpy's RandomState.random_sample (= rng.rand), bit for bit.
 * tc_gan/networks/ssn.py:434-439 draws `zs = rng.rand(batchsize, 2N, 2N)` from the RandomState the GAN shares with its
 * minibatch sampler (stream order networks/cwgan.py:438-481) and hands it to Theano in floatX (utils/theanoutils.py:9-16:
 * fp64 -> fp32 by round to nearest even).  numpy (pinned 1.13.1, requirements-conda.txt:46) implements RandomState as
 * randomkit's MT19937; this call continues that generator from the caller's state:
 *   key[624], *pos   numpy's `RandomState.get_state()[1:3]` (HOST, in/out; 0 <= pos <= 624).  On return they are the state
 *                    numpy itself would have after `random_sample(total)`: pass them to `set_state` and the next host draw
 *                    (`choice`, `rand`) continues exactly as in the reference.  The call returns once that state is known; it
 *                    waits for a short chain on a stream of the library's own, never for `stream`.
 *   total            doubles the draw consumes (2 words each: (a >> 5, b >> 6) -> (a 2^26 + b) / 2^53)
 *   skip, count      doubles [skip, skip + count) of the draw are written to out[0 .. count) (device) on `stream`; the rest is
 *                    not generated -- a rank of a data-parallel job passes its own rows of the global draw.  count = 0 only
 *                    advances the state.
 * _f32 rounds each double to the nearest float (ties to even), as numpy's astype(float32) does.  Any slice costs jump-ahead
 * by precomputed polynomials (Haramoto et al. 2008; ssn_mt19937_poly.h), built at the first call (tens of ms per level).
 * ssn_mt19937_jump_poly is the host-side arithmetic alone, for tests: bits[313] = t^(624 nblocks) mod the characteristic
 * polynomial; needs no device.
 */
int ssn_mt19937_random_sample_f32(unsigned int *key, int *pos, unsigned long long total, unsigned long long skip,
                                  unsigned long long count, float *out, void *stream);
int ssn_mt19937_random_sample_f64(unsigned int *key, int *pos, unsigned long long total, unsigned long long skip,
                                  unsigned long long count, double *out, void *stream);
int ssn_mt19937_jump_poly(unsigned long long nblocks, unsigned long long *bits);
/* The same draw in two halves, for a caller that has launches to queue before it next needs its generator: _begin launches
 * everything (key / pos are read, not written) and returns a ticket at once; _finish(ticket) waits for the state after the
 * draw -- one small launch on the library's own stream -- and writes it to key / pos.  A ticket is finished at most once
 * (a second time: invalid argument) and may be finished any time later, after any number of other draws.  ssn_mt19937_random_sample_* = _begin followed by _finish. */
int ssn_mt19937_random_sample_begin_f32(const unsigned int *key, int pos, unsigned long long total, unsigned long long skip,
                                        unsigned long long count, float *out, void *stream, int *ticket);
int ssn_mt19937_random_sample_begin_f64(const unsigned int *key, int pos, unsigned long long total, unsigned long long skip,
                                        unsigned long long count, double *out, void *stream, int *ticket);
int ssn_mt19937_random_sample_finish(int ticket, unsigned int *key, int *pos);
/* ssn_mt19937_random_sample_begin_f32 with W = make_W_with_x(z; J, D, S) (ssn_build_w_f32's arithmetic, the same bits) formed in
 * the generation kernel itself: the draw is z[B_total][2N][2N] of the caller's stream, models b0 .. b0 + nb - 1 of it are this
 * call's (a rank's rows), W: device [nb][2N][2N]; z: device [nb][2N][2N] to keep the numbers (the generator update's chain rule
 * reads them) or NULL -- then they never touch memory.  J, D, S: HOST float[4].  Finish with ssn_mt19937_random_sample_finish. */
int ssn_build_w_mt19937_begin_f32(const unsigned int *key, int pos, int B_total, int b0, int nb, const float *J, const float *D,
                                  const float *S, float *W, float *z, int N, void *stream, int *ticket);
/* The two draws above followed IN THE SAME CALL by what the reference's heterogeneous-input models draw right behind zs
 * (tc_gan/networks/ssn.py:710-720, 764-767: `zs_in`), so that the host does not have to fetch the state between the two:
 *   tail_kind 1      rng.choice(2, n) * 2 - 1: one 32-bit output per element, its low bit (numpy's masked rejection with
 *                    mask 1 rejects nothing: `_rand_int64` / `random_bounded_uint64_fill` with rng = 1), as -1.f / 1.f
 *   tail_kind 2      rng.rand(n) * 2 - 1: one double per element, 2 x - 1 exact in double, then rounded to the nearest float
 *   tail_total       elements the tail consumes; [tail_skip, tail_skip + tail_count) of them go to tail_out (device, fp32)
 * The ticket's state is the one behind the tail.  ssn_build_w_mt19937_tail_begin_f32: the tail is zs_in[B_total][2N], rows
 * b0 .. b0 + nb - 1 go to zin: device [nb][2N].  Windows that lie far apart in the stream (a rank's rows) get a launch each. */
int ssn_mt19937_random_sample_tail_begin_f32(const unsigned int *key, int pos, unsigned long long total, unsigned long long skip,
                                             unsigned long long count, float *out, int tail_kind, unsigned long long tail_total,
                                             unsigned long long tail_skip, unsigned long long tail_count, float *tail_out,
                                             void *stream, int *ticket);
int ssn_build_w_mt19937_tail_begin_f32(const unsigned int *key, int pos, int B_total, int b0, int nb, const float *J, const float *D,
                                       const float *S, float *W, float *z, int N, int tail_kind, float *zin, void *stream, int *ticket);
/* Host arithmetic of a draw alone (no device): out[7] = {pos after the draw, regenerations of the key up to then, blocks per
 * segment, first and last segment this call generates, first and last block that holds a wanted word} for the given pos /
 * total / skip / count -- what the CPU tests check against numpy's own positions, rank by rank. */
int ssn_mt19937_plan(int pos, unsigned long long total, unsigned long long skip, unsigned long long count, long *out);
/* ... of a draw with a tail (ssn_mt19937_random_sample_tail_begin_f32): the position and the blocks cover the tail's words too */
int ssn_mt19937_plan_tail(int pos, unsigned long long total, unsigned long long skip, unsigned long long count, int tail_kind,
                          unsigned long long tail_total, unsigned long long tail_skip, unsigned long long tail_count, long *out);

/* ---- Scoring the checkpoints of a run (analyzers/distdiff.py; csrc/ssn_score.hip) ---------------------------------
 * S recorded parameter sets share one noise draw and run as one forward batch of S B draws (set s owns draws [s B, (s + 1) B));
 * the tuning curves are reduced to two-sample Kolmogorov-Smirnov statistics against the truth on the device.
 * ssn_build_w_table_f32: W[s][b] = make_W_with_x(z[b]; J_s, D_s, S_s) for s < S, b < B; jds_table: DEVICE float[S][12] (J, D, S
 *   row-major, the layout of ssn_build_w_devparams_f32), z: device [B][2N][2N], W: device [S][B][2N][2N].  z is read once per
 *   draw.  The arithmetic of ssn_build_w_f32: the same values give the same bits.
 * ssn_tc_features_f32: tc: device [rows][NC NB Q], column (c NB + b) Q + q (the order of networks/utils.gridify_tc_samples with
 *   Q = cell types x probes); feat: device [rows][4][NC Q]: of every curve (c, q) over its NB bandwidths, in this order,
 *   maxrate = max_b tc, si = 1 - tc[NB - 1] / maxrate, prefbw = first index of the maximum, ipr = (sum tc)^2 / (NB sum tc^2).
 * ssn_ks_columns_f32: x: device [S][B][C]; truth_sorted: device [C][T], every column ascending with its m[c] finite values
 *   first (m: device int[C]).  n[s][c] = number of finite values among x[s][.][c] (the others are left out), num[s][c] =
 *   max over the pooled points v of |#{x <= v} m - #{t <= v} n|, so that the KS statistic is num / (n m); n = 0 or m = 0
 *   gives num = 0.  B <= SSN_KS_MAX_DRAWS (one workgroup sorts a column in LDS); more is refused. */
#define SSN_KS_MAX_DRAWS 16384
int ssn_build_w_table_f32(const float *z, const float *jds_table, float *W, int S, int B, int N, void *stream);
int ssn_tc_features_f32(const float *tc, float *feat, long rows, int NC, int NB, int Q, void *stream);
int ssn_ks_columns_f32(const float *x, const float *truth_sorted, const int *m, int S, int B, int C, int T, int *n,
                       long long *num, void *stream);

/* ---- Wasserstein distances of the scored checkpoints (analyzers/distdiff.py, wasserstein=True; csrc/ssn_wdist.hip) ----
 * The first Wasserstein distance of two samples on the line is the integral of |F_x - F_t|; with the counts the KS kernel
 * already has it is a sum over the pooled points, kept -- like num -- before the division by n m.
 * ssn_ks_w1_columns_f32: the arguments, the refusals and n, num of ssn_ks_columns_f32 (the same integers), and
 *   wnum[s][c] = sum_{k < K} gap_k w_k over the distinct finite values p_0 < p_1 < ... < p_K of the pooled sample (a value that
 *   occurs several times, in one sample or in both, is one point):
 *     gap_k = (double) p_{k+1} - (double) p_k,   w_k = (double) |#{x <= p_k} m - #{t <= p_k} n|   (an integer, 64-bit arithmetic)
 *   so that W1 = wnum / (n m), in the unit of x; n = 0 or m = 0 gives wnum = 0.  Every product is rounded once to fp64; the sum
 *   is in fp64 in an order the launch geometry fixes (per thread in index order, lanes 32, 16, ... 1 apart, the four waves in
 *   order), without atomics: two calls give the same bits.  All terms are non-negative, a product and a partial sum carry one
 *   rounding each and there are at most n + m terms: |wnum - exact| <= (n + m + 2) 2^-52 exact.  Where every gap, product and
 *   partial sum is representable (values on a lattice) wnum is exact.
 * ssn_project_rows_f32: out[r][l] = (float) acc with acc = 0 and, for c = 0 .. C - 1 in this order,
 *   acc = fma((double) x[r ldx + c], (double) theta[l C + c], acc): the products of two floats are exact in fp64, so this is the
 *   sequential fp64 sum of exact products, rounded to float at the end.  x: device [rows][ldx] of which the first C of a row
 *   are read (ldx >= C), theta: device [L][C], out: device [rows][L].  A non-finite x makes every projection of its row
 *   non-finite.  L <= SSN_W1_MAX_DIRECTIONS; more, a negative size, ldx < C or a null pointer is refused; rows == 0 or L == 0
 *   is success. */
#define SSN_W1_MAX_DIRECTIONS 4096
int ssn_ks_w1_columns_f32(const float *x, const float *truth_sorted, const int *m, int S, int B, int C, int T, int *n,
                          long long *num, double *wnum, void *stream);
int ssn_project_rows_f32(const float *x, long rows, int ldx, int C, const float *theta, int L, float *out, void *stream);

/* ---- Sliced Wasserstein loss of a minibatch and its gradient (networks/sliced_wasserstein.py; csrc/ssn_swd.hip) ----
 * px, py: device [B][L], the projections (ssn_project_rows_f32) of B generated rows and of B truth rows onto L directions.
 * ssn_swd_match_f32: for every direction l the pairs (px[b][l], b) are sorted ascending by value, ties by row index b -- the
 *   comparison is the float comparison, -0 counts as +0 (numpy's argsort(kind='stable')) -- and py[.][l] is sorted ascending.
 *   With u_i, v_i the i-th sorted values and b_i the row that holds u_i, d_i = (double) u_i - (double) v_i, and for power p:
 *     loss_l[l] = (sum_i |d_i|^p) / B        in fp64: |d_i| is exact, every product d_i d_i is rounded once, the sum runs in an
 *                                            order the launch geometry fixes (per thread in index order, lanes 32, 16, ... 1
 *                                            apart, the four waves in order), without atomics: two calls give the same bits.
 *                                            All terms are non-negative: |loss_l - exact| <= (B + 2) 2^-52 exact, and the value
 *                                            is exact where every term and partial sum is representable and B is a power of two;
 *     coef[b_i][l] = (float) (sign(d_i) inv)     p = 1, sign(0) = 0
 *     coef[b_i][l] = (float) ((2.0 d_i) inv)     p = 2,         with inv = 1.0 / ((double) L (double) B):
 *   the derivative of (1/L) sum_l loss_l[l] by px[b][l].  For p = 1 loss_l[l] is the W1 of the two columns, the unit of
 *   ssn_ks_w1_columns_f32's wnum / (n m).  A column of px or py that holds a value which is not finite gives loss_l[l] = NaN and
 *   coef[.][l] = NaN (found before the sort).  coef: device [B][L], loss_l: device double[L].
 *   B <= SSN_SWD_MAX_BATCH (one workgroup sorts 64-bit keys of px and the values of py in 48 KiB of LDS, padded to a power of
 *   two) and L <= SSN_W1_MAX_DIRECTIONS; more, a negative size, a power other than 1 or 2 or a null pointer is refused; B == 0
 *   or L == 0 is success and writes nothing.
 * ssn_swd_backproject_f32: gx[b][c] = (float) acc with acc = 0 and, for l = 0 .. L - 1 in this order,
 *   acc = fma((double) coef[b L + l], (double) theta[l D + c], acc): the products of two floats are exact in fp64, so this is the
 *   sequential fp64 sum of exact products, rounded to float at the end -- the derivative of the loss by x[b][c] where
 *   px = x theta^T.  theta: device [L][D], gx: device [B][D].  A NaN column of coef makes all of gx NaN.  L == 0 writes zeros;
 *   B == 0 or D == 0 is success and writes nothing; L above the limit, a negative size or a null pointer is refused. */
#define SSN_SWD_MAX_BATCH 4096
int ssn_swd_match_f32(const float *px, const float *py, int B, int L, int power, float *coef, double *loss_l, void *stream);
int ssn_swd_backproject_f32(const float *coef, const float *theta, int B, int L, int D, float *gx, void *stream);

/* ---- 6c. Ensembles of sliced Wasserstein runs (networks/sliced_wasserstein_ensemble.py; csrc/ssn_ens_swd.hip) ----
 * K independent runs of the loss above in one launch each, whatever K is (ssn_ens_swd_match_f32: two, the match and the sum
 * l0).  Member k owns rows [k B, (k + 1) B) of x[K B][D] (generated) and y[K B][D] (its truth minibatch), its own directions
 * theta[k][L][D] and its own power[k] in {1, 2}; L, B and D are shared.  Every sum of a member runs over its own rows in the
 * single run's order: the kernels call the device functions the single-run kernels call, so the outputs of member k are THE BITS
 * ssn_project_rows_f32, ssn_swd_match_f32 and ssn_swd_backproject_f32 give for that member alone (B, L, D, its theta, its
 * power), on every launch.  No atomics.
 * ssn_ens_swd_project_f32: px, py: device [K B][L], the projections of x and of y on the member's theta; one launch for both
 *   samples and all members.  D == 0 writes zeros.
 * ssn_ens_swd_match_f32: coef: device [K B][L], loss_l: device double[K][L], l0: device double[K] with
 *     l0[k] = (sum_l loss_l[k][l]) / L,   a sequential fp64 sum in index order, no contraction: numpy's cumsum(loss_l[k])[-1] / L;
 *   inv = 1 / (L B) with B of ONE member.  power: HOST int[K], read before the call returns.  A value that is not finite in
 *   member k's column l gives NaN for loss_l[k][l], coef[k B .. (k + 1) B)[l] and l0[k] and touches nothing of another member.
 *   form: SSN_SWD_FORM_AUTO (the wave form where B <= SSN_SWD_WAVE_MAX_BATCH, else the general form), SSN_SWD_FORM_GENERAL (one
 *   workgroup per (direction, member), the LDS bitonic network of ssn_swd_match_f32) or SSN_SWD_FORM_WAVE (one wave64 per
 *   (member, direction) column, keys and values in registers, the same network over cross-lane moves; B <= 64 or refused).
 *   Both forms give the same bits.
 * ssn_ens_swd_backproject_f32: gx: device [K B][D] from coef and the member's theta.  L == 0 writes zeros.
 * Refused (ssn_last_error names it): K > SSN_ENS_SWD_MAX_MEMBERS, B > SSN_SWD_MAX_BATCH, L > SSN_W1_MAX_DIRECTIONS, a power other
 *   than 1 or 2, an unknown form, a negative size, a null pointer.  K, B or L == 0 is success and writes nothing.
 * ssn_ens_gen_grads_l0_f32: ssn_ens_gen_grads_f32 with L0 of member k taken from l0[k] (device double[K]) instead of formed
 *   from moments: a->D == 0, a->data_moments and a->weights NULL (else refused).  The record row of ssn_ens_record_doubles(0, P):
 *   [0] L0, [1] dynamics_penalty, [2] rate_penalty, [3] loss = L0 + costs[k][0] dyn + costs[k][1] rate, [4 .. 4 + P) the new
 *   parameters, then the P gradients.  Gradients and penalties are the bits of ssn_ens_gen_grads_f32. */
#define SSN_ENS_SWD_MAX_MEMBERS 2048
#define SSN_SWD_WAVE_MAX_BATCH 64
#define SSN_SWD_FORM_AUTO 0
#define SSN_SWD_FORM_GENERAL 1
#define SSN_SWD_FORM_WAVE 2
int ssn_ens_swd_project_f32(const float *x, const float *y, const float *theta, int K, int B, int L, int D, float *px, float *py,
                            void *stream);
int ssn_ens_swd_match_f32(const float *px, const float *py, const int *power, int K, int B, int L, int form, float *coef,
                          double *loss_l, double *l0, void *stream);
int ssn_ens_swd_backproject_f32(const float *coef, const float *theta, int K, int B, int L, int D, float *gx, void *stream);
int ssn_ens_gen_grads_l0_f32(const ssn_ens_grads *a, const double *l0, void *stream);

/* ---- Rejection sampling of fixed points on the device (ssnode.sample_tuning_curves_table; csrc/ssn_fpsample.hip) ----
 * A parameter sets see the same stream of candidate draws; every (set, candidate) pair is solved for NB stimuli by
 * ssn_solve_batch_* (the A R pairs as its batch, set-major), and the first NZ candidates of a set, in stream order, whose solves
 * all succeed are kept: the rule of ssnode.find_fixed_points, with the states staying on the device.
 * ssn_build_w_table_f64: ssn_build_w_table_f32 in fp64 (jds_table: DEVICE double[S][12]): the bits of ssn_build_w_f64 per set.
 * ssn_fp_select_f64 / _f32: one round of R candidates for A sets, two launches on `stream`.
 *   codes: device [A][R][NB] and x: device [A][R][NB][M], as the solver left them.  A (candidate, stimulus) pair fails with its
 *   code, and with code 1 where the code is 0 but one of its M values is not finite.  verdict[a][b] (device int[A][R], a
 *   workspace that is left filled) = 0 where no stimulus fails, else the failure code of the failing stimulus with the LARGEST
 *   index (the first one in reversed stimulus order).
 *   set_of: device int[A], the row of the arrays below that set a of this round owns (rows are distinct); cand0: the stream
 *   index of the round's first candidate; probes: device int[nprobe], the neurons whose rates are kept.  Per row, updated in
 *   place (the caller zeroes accepted / used / rejections, fills draw_index with -1 and out with NaN before the first round):
 *     out [.][NZ][NB nprobe]   row accepted' = accepted + rank of every newly accepted candidate: x[a][b][s][probes[p]] in
 *                              column s nprobe + p;
 *     accepted [.]             rows filled so far (at most NZ; a row that has NZ is left alone by later rounds);
 *     used [.]                 cand0 + R while the row is short, the stream index of its NZ-th success plus one once reached;
 *     rejections [.][2]        candidates with verdict 1 and 2 in front of the NZ-th success (other codes are not counted:
 *                              with the solver's codes, accepted + rejections[0] + rejections[1] == used);
 *     draw_index [.][NZ]       stream index of every accepted row.
 *   R <= ssn_fp_select_max_candidates() (one workgroup per set keeps the round's accepted indices in LDS); more, NZ < 1, odd M
 *   or a null pointer is refused.  A == 0 or R == 0 is success. */
int ssn_build_w_table_f64(const double *z, const double *jds_table, double *W, int S, int B, int N, void *stream);
int ssn_fp_select_max_candidates(void);
int ssn_fp_select_f64(const int *codes, const double *x, int A, int R, int NB, int M, const int *probes, int nprobe,
                      const int *set_of, int cand0, int NZ, int *verdict, double *out, int *accepted, int *used, int *rejections,
                      int *draw_index, void *stream);
int ssn_fp_select_f32(const int *codes, const float *x, int A, int R, int NB, int M, const int *probes, int nprobe,
                      const int *set_of, int cand0, int NZ, int *verdict, float *out, int *accepted, int *used, int *rejections,
                      int *draw_index, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSNODE_MI355X_H */

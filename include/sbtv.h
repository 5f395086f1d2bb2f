/*
 * sbtv.h — C-ABI of libsbtv.so: the MI355X (gfx950) implementation of the
 * FFT-convolution + TV-proximal inner loop of SALSA / FISTA / SAPG(MYULA).
 *
 * The reference (charles-kmc/Semi-blind-image-deblurring-problems-with-TV) is
 * pure MATLAB and has no FFI layer: its "operator API" is function handles
 * and name/value option lists.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference checkout).  A host
 * binds these with MATLAB loadlibrary/calllib (this header is plain C, no
 * mex.h), a MEX gateway, or Python ctypes — see INTEGRATION.md.
 *
 * Conventions
 *   - all image buffers are IEEE double, column-major (MATLAB layout):
 *     element (i,j) of image b lives at  buf[b*M*N + j*M + i],  M rows, N cols.
 *   - image sizes: 2 <= M, N <= 4096 for every entry point that applies the blur
 *     operator (SBTV_ERR_SIZE otherwise).  Powers of two from 16 take the tuned radix-2^k
 *     real-FFT kernels; any other size runs like the reference's fft2 closures do
 *     (utils/resize.m:1-12) through a chirp-z (Bluestein) complex transform, several
 *     times slower.  FISTA, SAPG / MYULA, max_eigenval, C-SALSA and CoRAL additionally
 *     need an even number of pixels.  The TV entry points (prox, TVnorm) accept any
 *     M >= 2, N >= 2 (even M takes the fused 16-byte-per-lane kernels, odd M a scalar
 *     one-iteration kernel).
 *   - `flags & SBTV_DEVICE_PTRS`: image buffers are device pointers on the
 *     context's GPU (no PCIe copies; asynchronous on the context stream).
 *     Otherwise they are host pointers and the call copies in/out and returns
 *     after the results are on the host.  Small option/result arrays
 *     (scalars per image, traces) are ALWAYS host pointers.
 *   - return value: 0 = ok; < 0 argument errors (mirror the reference's
 *     error() sites); > 0 HIP runtime errors.  sbtv_last_error() gives text.
 *     Nothing throws across the boundary.
 *   - one context = one GPU = one host thread at a time; sbtv_group (below) bundles one context per GPU behind
 *     one call for hosts that are a single process.
 */
#ifndef SBTV_H
#define SBTV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBTV_VERSION 100

/* flags */
#define SBTV_HOST_PTRS   0
#define SBTV_DEVICE_PTRS 1
/* sbtv_SAPG_algorithm only: */
#define SBTV_REDUCE_DEVICE  2   /* reduce_fn is an sbtv_allreduce_dev_fn (in-stream collective on a device buffer)  */
#define SBTV_SAPG_HOST_LOOP 4   /* parameter updates on the host, one synchronisation per iteration (the round-1 loop) */
/* sbtv_fista_tv only: */
#define SBTV_FISTA_EXACT_PROX 2 /* stop-rule kernel after every Chambolle launch (default: the launches of a prox run all
                                 * prox_iters iterations, the host applies the rule of chambolle_prox_TV_stop.m:131 over the
                                 * steps afterwards and repeats the solve with exact launches if it stopped early) */

/* status codes */
#define SBTV_OK                   0
#define SBTV_ERR_BADARG          -1   /* generic bad argument                                  */
#define SBTV_ERR_SIZE            -2   /* unsupported image size (outside 2..4096, or an odd pixel count where noted) */
#define SBTV_ERR_MAXITER         -3   /* chambolle: 'maxiter' missing  (chambolle_prox_TV_stop.m:95,131, quirk Q1) */
#define SBTV_ERR_DUALVARS        -4   /* 'Wrong size of the dual variables' (chambolle_prox_TV_stop.m:103)          */
#define SBTV_ERR_MODE            -5   /* 'The value of parameter mode must be 1 or 2' (A_wrapper.m:15)              */
#define SBTV_ERR_STOPCRITERION   -6   /* 'Unknown stopping criterion' (SALSA_v2.m:246; my_fista.m:45)               */
#define SBTV_ERR_INIT            -7   /* "Unknown 'Initialization' option" (SALSA_v2.m:382)                          */
#define SBTV_ERR_MISSING_AT      -8   /* 'The function handle for transpose of A is missing' (SALSA_v2.m:262)        */
#define SBTV_ERR_MISSING_LS      -9   /* '(A^T A + mu I)^(-1) must be specified' (SALSA_v2.m:296)                    */
#define SBTV_ERR_PSF            -10   /* bad PSF size / mask does not fit (conv2c.m:15)                               */
#define SBTV_ERR_NOMEM          -11
#define SBTV_ERR_NODEVICE       -12   /* no usable GPU: the library has NO CPU fallback                               */
#define SBTV_ERR_PEER           -14   /* shared-gradient chains: another rank reported an error through reduce_fn     */
#define SBTV_ERR_CANARY         -13   /* SBTV_CANARY=1: a kernel wrote outside its workspace (guard band damaged)     */

typedef struct sbtv_ctx sbtv_ctx;

/* ---- context ---------------------------------------------------------- */
int         sbtv_version(void);
/* Create a context on GPU `device`.  Fails with SBTV_ERR_NODEVICE when no
 * gfx950-capable device is visible (there is deliberately no CPU path). */
int         sbtv_ctx_create(int device, sbtv_ctx **out);
int         sbtv_ctx_destroy(sbtv_ctx *ctx);
const char *sbtv_last_error(const sbtv_ctx *ctx);   /* ctx may be NULL: global message */
/* Use an externally owned hipStream_t (e.g. torch's current stream). NULL = own stream. */
int         sbtv_ctx_set_stream(sbtv_ctx *ctx, void *hip_stream);
int         sbtv_ctx_sync(sbtv_ctx *ctx);
/* Lanes (no counterpart in the reference): a call with batch >= 2 independent items (the images of sbtv_SALSA_v2 /
 * sbtv_fista_tv / sbtv_CSALSA_v2 / sbtv_CoRAL_v2, the independent chains of sbtv_SAPG_algorithm) is dealt in two
 * contiguous halves to two internal contexts on the same GPU - own stream, workspaces and host thread each - so that the
 * launch tails and memory-bound passes of one half run under the Chambolle launches of the other (+15..20 % image-
 * iterations/s).  Results do not change: a batched call computes image k bit for bit like image k alone.
 *   mode 0 (default) independent items only;  1 never (one stream);  2 also shared-gradient chains (share_gradients = 1:
 *   the two halves then exchange their six gradient sums in-stream once per SAPG iteration, results equal to rounding).
 * The environment variable SBTV_LANES = 0 | 1 | 2 overrides the mode of every context.  With a caller-owned stream
 * (sbtv_ctx_set_stream) the call first waits for that stream, then runs on the lanes' own streams. */
int         sbtv_ctx_set_lanes(sbtv_ctx *ctx, int mode);
/* Operator-call counters: the reference's global `calls` (SALSA/callcounter.m:8-15). */
int         sbtv_callcounter_get(const sbtv_ctx *ctx, long long *calls);
int         sbtv_callcounter_reset(sbtv_ctx *ctx);
/* Timing of the most recent solver call, measured with HIP events on the
 * context stream: [0] total ms of the call on the device (set-up and iteration loop), [1] ms inside the
 * Chambolle iteration kernels, [2] number of Chambolle iteration launches,
 * [3] algorithmic bytes those launches moved (40 B/pixel/iteration). */
int         sbtv_last_timing(const sbtv_ctx *ctx, double out[4]);

/* raw device memory helpers so hosts without a GPU array type (MATLAB) can
 * keep buffers resident between calls */
int         sbtv_malloc(sbtv_ctx *ctx, size_t bytes, void **dptr);
int         sbtv_free(sbtv_ctx *ctx, void *dptr);
int         sbtv_memcpy_h2d(sbtv_ctx *ctx, void *dst, const void *src, size_t bytes);
int         sbtv_memcpy_d2h(sbtv_ctx *ctx, void *dst, const void *src, size_t bytes);

/* ---- a-1: TV proximal operator ----------------------------------------
 * Replaces  [f,px,py] = chambolle_prox_TV_stop(g,'lambda',L,'maxiter',K,
 *                        'tol',t,'tau',T,'dualvars',[px py])
 * (utils/chambolle_prox_TV_stop.m:1-166), batched over `batch` images.
 *   lambda[batch]   regularisation weight per image
 *   maxiter         REQUIRED, > 0 (quirk Q1) else SBTV_ERR_MAXITER
 *   tol, tau        reference defaults 1e-3, 0.249 (:77-78)
 *   warm_start      0: px=py=0 (:68-69); 1: px,py hold the dual variables on entry (:99-107)
 *   px,py,f         M*N*batch each; px,py always written; f may be NULL
 *   k_out[batch]    iterations actually run;  err_out[batch] last `err` (:128)
 */
int sbtv_chambolle_prox_TV_stop(sbtv_ctx *ctx, const double *g, int M, int N, int batch,
                                const double *lambda, int maxiter, double tol, double tau,
                                int warm_start, double *px, double *py, double *f,
                                int *k_out, double *err_out, int flags);

/* ---- a-2: periodic isotropic TV ----------------------------------------
 * Replaces  TVnorm(x)  (utils/TVnorm.m:2; SALSA/diffh.m, diffv.m, conv2c.m). out[batch]. */
int sbtv_TVnorm(sbtv_ctx *ctx, const double *x, int M, int N, int batch, double *out, int flags);

/* ---- a-3/a-4: circular blur operator from PSF taps ----------------------
 * The reference builds A, AT, dA/dp, invLS as FFT closures over
 * resize(h) = fft2 of the taille x taille taps zero-padded into the TOP-LEFT
 * corner (utils/resize.m:1-12; run_Gaussian_demo.m:126-139,224-225).  Here a
 * PSF is its taps (column-major taille x taille, taille <= 15, per image).
 *
 * sbtv_A_wrapper replaces A_wrapper(A,AT,x,M1,N1,M2,N2,mode) (SALSA/A_wrapper.m:5-17)
 * for the closures of the demos:
 *   mode 1: A x   = real(ifft2( H        .* fft2(x)))      run_Gaussian_demo.m:136
 *   mode 2: AT x  = real(ifft2( conj(H)  .* fft2(x)))      run_Gaussian_demo.m:137
 *   mode 3: dA x  = same as mode 1 (pass the derivative taps)   :138-139
 *   mode 9: invLS = real(ifft2( fft2(x) ./ (abs(H).^2 + mu)))   :224-225
 * other modes -> SBTV_ERR_MODE.  Each call bumps the call counter by `batch`.
 */
int sbtv_A_wrapper(sbtv_ctx *ctx, const double *taps, int taille, const double *mu,
                   const double *x, double *out, int M, int N, int batch, int mode, int flags);

/* PSF tap builders (host arithmetic, exactly the reference formulas).
 * kind 0 gaussian  p = {w1, w2, phi}  utils/Gaussian_psf.m:2-19, Sum_gauss_psf.m, diff_fftgaus_w1/w2.m
 * kind 1 moffat    p = {alpha, beta}  utils/psf_moffat.m:2-20, sum_mof_psf.m, diff_moffat_alpha/beta.m
 * kind 2 laplace   p = {b}            utils/psf_laplace.m:1-13, sum_lap_psf.m, diff_laplace_b.m
 * taps, d0, d1: taille*taille doubles (column-major); d0/d1 may be NULL. */
#define SBTV_PSF_GAUSSIAN 0
#define SBTV_PSF_MOFFAT   1
#define SBTV_PSF_LAPLACE  2
int sbtv_psf_taps(int kind, int taille, const double *p, double *taps, double *d0, double *d1);

/* The PSF-tracking trace results.err_psf of the SAPG loops (SAPG_algorithm_Guassian.m:146,203-204, _moffat.m:204-205,
 * _laplace.m:136,190-191):  out[i] = l2(psf(params(i)), psf(p_true)) with utils/l2.m = norm(.)^2 of the MATRIX
 * (spectral norm, quirk Q9).  ps = [first-parameter trace (n) | second-parameter trace (n)], host arrays; the
 * Gaussian pairs w1s(i) with w2s(i-1) (quirk Q8), the Moffat's first entry stays 0 as in the reference. */
int sbtv_err_psf(int kind, int taille, const double *ps, int n, const double *p_true, double phi, double *out);

/* Packed half-spectrum of a real image (debug / test entry for the FFT
 * kernels): out is (M/2) x N complex, column-major, interleaved re/im; row 0
 * holds X[0,l] + i*X[M/2,l].  inverse=1 maps it back (scaled like ifft2). */
int sbtv_rfft2_packed(sbtv_ctx *ctx, const double *in, double *out, int M, int N, int batch,
                      int inverse, int flags);

/* ---- a-7: SALSA_v2 -------------------------------------------------------
 * Replaces  [x,numA,numAt,objective,distance,times,mses] = SALSA_v2(y,A,tau,
 *   'MU',mu,'AT',AT,'StopCriterion',c,'True_x',x,'ToleranceA',tol,'MAXITERA',n,
 *   'TVINITIALIZATION',1,'TViters',k,'LS',invLS,...)   (SALSA/SALSA_v2.m:156-494)
 * with A/AT/invLS the FFT closures defined by `taps` (run_Gaussian_demo.m:215-242).
 * Only the TV path ('TVINITIALIZATION' = 1) exists: like the reference (:318-320,
 * quirk Q7) user Psi/Phi are ignored in that mode.
 */
typedef struct sbtv_salsa_opts {
    int    stopcriterion;    /* 1,2,3  (SALSA_v2.m:245-247,456-469)                 */
    int    maxiter;          /* 'MAXITERA'  default 10000 (:173)                    */
    int    TViters;          /* 'TVITERS'   default 5 (:181)                        */
    int    initialization;   /* 0 zeros (:369), 2 AT*y (:373), 33333 x_init given   */
    int    compute_mse;      /* 1 when 'TRUE_X' given (:227-229)                    */
    int    speculate;        /* bit 0 (default 1): the host evaluates the outer stop rule one iteration late while the
                              * next iteration already runs (0: it waits for every iteration).
                              * bit 1: never launch the TV prox optimistically.  By default the Chambolle launches of an
                              * outer iteration run all TViters iterations without stop-rule kernels and the rule
                              * (chambolle_prox_TV_stop.m:131) is applied over those steps at the end of the iteration;
                              * if it fired before the last one the whole solve is repeated with exact launches, so the
                              * result is always that of the exact rule (TViters <= 10, even M). */
    double tolA;             /* 'TOLERANCEA' default 1e-3 (:178)                    */
    double chambolle_tol;    /* 1e-3  (chambolle_prox_TV_stop.m:78)                 */
    double chambolle_tau;    /* 0.249 (chambolle_prox_TV_stop.m:77)                 */
} sbtv_salsa_opts;

void sbtv_salsa_opts_default(sbtv_salsa_opts *o);

/*   y, true_x, x_init, x_out : M*N*batch images (true_x / x_init may be NULL)
 *   taps[batch*taille^2], tau[batch], mu[batch]            (host arrays)
 *   objective[batch*(maxiter+1)], distance[batch*maxiter], times[batch*(maxiter+1)],
 *   mses[batch*(maxiter+1)]  (host arrays, any may be NULL; row b starts at b*(maxiter+1)
 *   resp. b*maxiter);  numA, numAt, n_outer: [batch] (host, may be NULL)
 *   Images in a batch iterate in lock-step; an image that met its stop rule is
 *   frozen (its x no longer changes) while the others continue.
 *   x_out may overlap an input (then it is written once, at the end); a device-resident
 *   x_out that overlaps none is also written by the iteration numbered maxiter, so its
 *   contents are undefined until the call returns. */
int sbtv_SALSA_v2(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                  const double *taps, int taille, const double *tau, const double *mu,
                  const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                  double *x_out, double *objective, double *distance, double *times, double *mses,
                  int *numA, int *numAt, int *n_outer, int flags);

/* ---- f-3: the other ADMM front-ends over the same kernels ----------------
 * (never called by the reference's demos)  Only the TV paths exist
 * ('TVINITIALIZATION*' = 1, P/PT = identity) in these two entries; with the wavelet frame as P / PT see sbtv_CSALSA_wavelet and
 * sbtv_CoRAL_wavelet below.  Images of a batch are solved one after another.
 *
 * sbtv_CSALSA_v2 replaces
 *   [x,numA,numAt,objective,distance1,distance2,criterion,times,mses] = csalsa(y,A,mu1,mu2,sigma,
 *      'AT',AT,'LS',invLS,'TVINITIALIZATION',1,'TVITERS',k,'STOPCRITERION',c,'TOLERANCEA',tol,
 *      'MAXITERA',n,'CONTINUATIONFACTOR',delta,'EPSILON',eps,...)   (SALSA/CSALSA_v2.m:160-561)
 * with invLS(r,mu) = real(ifft2(fft2(r)./(|H|^2+mu))) (:116 of its help, called as invLS(r,mu1) :471).
 * opts: stopcriterion 1..3 (default of the reference: 3), maxiter, TViters, initialization, tolA and the
 * Chambolle knobs are used; `speculate` as for sbtv_SALSA_v2 (bit 0: the host evaluates the stop rule one iteration late,
 * bit 1: never launch the TV prox optimistically); a continuation factor != 1 selects exact launches and no lag.  Traces are 1-based like the reference: entry 0 is the
 * state before the loop, the loop runs outer = 2..maxiter (:461).  All trace rows have maxiter entries.
 * epsilon[b] = 0 selects sqrt(numel(y)+8*sqrt(numel(y)))*sigma[b] (:413).  n_outer[b] = last `outer`. */
int sbtv_CSALSA_v2(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                   const double *taps, int taille, const double *mu1, const double *mu2,
                   const double *sigma, const double *epsilon, double continuationfactor,
                   const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                   double *x_out, double *objective, double *distance1, double *distance2,
                   double *criterion, double *times, double *mses,
                   int *numA, int *numAt, int *n_outer, int flags);

/* sbtv_CoRAL_v2 replaces
 *   [x,numA,numAt,objective,distance,times,mses] = CoRAL(y,A,tau1,tau2,'MU1',mu1,'MU2',mu2,'AT',AT,
 *      'LS',invLS,'TVINITIALIZATION1',1,'TVITERS1',k1,'TVINITIALIZATION2',1,'TVITERS2',k2,...)
 *   (SALSA/CoRAL_v2.m:2-476), invLS(r) = real(ifft2(fft2(r)./(|H|^2+mu_ls))), mu_ls = mu1+mu2 (:137)
 * when mu_ls is NULL.  opts->TViters is TViters1; TViters2 is a separate argument.
 * objective/times/mses: [batch*(maxiter+1)]; distance: [batch*maxiter*2], entry (outer-1)*2+{0,1}. */
int sbtv_CoRAL_v2(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                  const double *taps, int taille, const double *tau1, const double *tau2,
                  const double *mu1, const double *mu2, const double *mu_ls, int TViters2,
                  const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                  double *x_out, double *objective, double *distance, double *times, double *mses,
                  int *numA, int *numAt, int *n_outer, int flags);

/* ---- masked-observation SALSA: unknown boundaries and missing pixels ------------------------------------------------
 * The SALSA toolbox knows a mask OR a blur ('MASK', 1: SALSA/SALSA.m:103-104,308-312,463-464 and
 * SALSA/csalsa.m:112-113,349-352,510-511 solve with 1 ./ (mu + mask)); a mask OF a blur has no counterpart in the
 * reference.  This entry is the ADMM of Almeida & Figueiredo ("Deconvolving images with unknown boundaries using the
 * alternating direction method of multipliers", IEEE TIP 2013) on the kernels of sbtv_SALSA_v2:
 *     minimise over x   0.5 * sum( m .* (B x - y).^2 ) + tau * TV(x)
 * B: circular blur of `taps` (top-left embedding, utils/resize.m), m = mask: M*N*batch non-negative weights like y (0 = not
 * observed, 1 = observed, other values weigh a pixel); y enters only as m .* y, its values under m = 0 must be finite.
 * With the splits u = x, v = B x and scaled multipliers bu, bv in SALSA_v2's sign convention (SALSA/SALSA_v2.m:429-440)
 * one outer iteration is
 *     u  = chambolle_prox_TV_stop(x - bu, 'lambda', tau/mu1, 'maxiter', TViters, 'dualvars', [pux puy])
 *     v  = (m .* y + mu2 * (Bx - bv)) ./ (m + mu2)
 *     X  = (mu1 * fft2(u + bu) + mu2 * conj(H) .* fft2(v + bv)) ./ (mu1 + mu2 * abs(H).^2)
 *     x  = real(ifft2(X));    Bx = real(ifft2(H .* X))
 *     bu = bu + (u - x);      bv = bv + (v - Bx)
 *     objective(outer+1) = 0.5 * sum(m .* (Bx - y).^2) + tau * TVnorm(u)
 * Start: x by opts->initialization (0 zeros, 2 B'(m .* y), 33333 x_init), Bx = B x, u = x, v = Bx, bu = bv = 0, zero duals;
 * objective(1) from that state.  Stop rules 1, 2, 3 as SALSA/SALSA_v2.m:453-482 (from the second outer iteration on).
 * objective / times / mses: [batch*(maxiter+1)] (mses against true_x over all M*N pixels, SALSA_v2.m:446-449);
 * distance: [batch*maxiter*2], entry (outer-1)*2 + {0,1} = ||x-u|| / sqrt(||x||^2+||u||^2), ||Bx-v|| / sqrt(||Bx||^2+||v||^2);
 * numA / numAt count the applications of B / B' as the iteration is written: numA = 1 (the start's B x) + one per outer
 * iteration (H .* X), numAt = one per outer iteration (conj(H) .* fft2(v + bv)) + 1 when initialization = 2.
 * mu2 decides the speed, not the answer; 0.1 is the Python mirror's default (measured on one problem with pixel values
 * in 0..255).  `speculate` as for sbtv_SALSA_v2; images of a batch are solved one after another, image k bit for bit as alone.
 * Errors before any GPU work: mask == NULL, mu1[b] <= 0, mu2[b] <= 0 -> SBTV_ERR_BADARG; odd pixel count -> SBTV_ERR_SIZE;
 * stop criterion and initialization as sbtv_SALSA_v2.  With SBTV_HOST_PTRS a mask with a negative or non-finite entry is
 * rejected (SBTV_ERR_BADARG); a device-resident mask (it lives where y lives) is the caller's responsibility.
 * The samplers of the same likelihood, which estimate the tau, the PSF parameters and the sigma2 this entry needs, are
 * sbtv_myula_masked and sbtv_SAPG_masked below. */
int sbtv_SALSA_masked(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch,
                      const double *taps, int taille, const double *tau, const double *mu1, const double *mu2,
                      const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                      double *x_out, double *objective, double *distance, double *times, double *mses,
                      int *numA, int *numAt, int *n_outer, int flags);

/* ---- wavelet-l1 deconvolution: the redundant wavelet frame and its SALSA driver ----------------------------------
 * Replaces mrdwt_TI2D / mirdwt_TI2D / soft of the reference (SALSA/mrdwt_TI2D.m, mirdwt_TI2D.m, soft.m) and the solve of
 * SALSA/run_deblur_synthesis_L1.m:160-180 (SALSA_v2 with 'Psi' / 'LS').  The Rice Wavelet Toolbox MEX behind the reference's
 * two wrappers is not shipped (SALSA/mrdwt.m is a comment block); the transform is defined here.
 *
 * h: orthonormal scaling filter of even length hlen = K, 2 <= K <= 8, sum(h) = sqrt(2); h0 = h, h1[k] = (-1)^k h[K-1-k].
 * J = levels - 1 decomposition steps (the reference's convention: levels = 4 gives 10 bands).  Level j = 1..J, stride
 * s = 2^(j-1), along one dimension of length n with circular indices:
 *     lo[i] = (1/sqrt 2) sum_k h0[k] a[(i + s k) mod n],     hi[i] = (1/sqrt 2) sum_k h1[k] a[(i + s k) mod n]
 * first along dimension 1 (the contiguous row index of the column-major image), then along dimension 2.  Level j turns the
 * approximation a_{j-1} (a_0 = x) into a_j = (lo, lo) and the details LH, HL, HH (first letter: the filter along dimension 1).
 * z holds 3J+1 consecutive M x N column-major images per input image: band 0 = a_J, bands 1+3(j-1) .. 3+3(j-1) = LH, HL, HH
 * of level j; in memory the reference's M x (3J+1)N matrix [temp1 temp2] with the rescaling of mrdwt_TI2D.m:19-23 applied
 * (the 1/sqrt 2 per dimension).  The 1-D convention reproduces the example of SALSA/mrdwt.m:38-40.
 * sbtv_mrdwt_TI2D is the analysis operator W', sbtv_mirdwt_TI2D the synthesis operator W, its exact adjoint (transposed
 * filters, index (i - s k) mod n).  For an orthonormal h the frame is Parseval at every image size: W W' = I, ||W'x|| = ||x||.
 * Any M, N with (K-1) 2^(J-1) < min(M, N) (a tap wraps at most once), else SBTV_ERR_SIZE; K odd or outside 2..8,
 * levels < 2, h == NULL -> SBTV_ERR_BADARG; all refused before any GPU work.  The bare transforms accept any h.
 * One kernel launch per level: 5 * M*N * 8 bytes of traffic each. */
int sbtv_mrdwt_TI2D(sbtv_ctx *ctx, const double *x, int M, int N, int batch,
                    const double *h, int hlen, int levels, double *z, int flags);
int sbtv_mirdwt_TI2D(sbtv_ctx *ctx, const double *z, int M, int N, int batch,
                     const double *h, int hlen, int levels, double *x, int flags);
/* out = soft(x, T) = sign(x) .* max(abs(x) - T, 0) (SALSA/soft.m) on `batch` arrays of M*N doubles, T[batch] >= 0 (host);
 * T = 0 passes x through. */
int sbtv_soft(sbtv_ctx *ctx, const double *x, int M, int N, int batch, const double *T, double *out, int flags);
/* min over xw  0.5 ||y - B W xw||^2 + tau ||xw||_1  (B: circular blur of `taps`), as SALSA/SALSA_v2.m:389-494 solves it with
 * TVINITIALIZATION = 0, Psi = soft, Phi = l1, A = B W, AT = W' B' and the invLS of run_deblur_synthesis_L1.m:169-170.
 * With W W' = I one outer iteration of that is exactly
 *     u  = soft(xw - bu, tau/mu) ;  s = u + bu ;  z = W s
 *     X  = (conj(H) .* fft2(y) + mu * fft2(z)) ./ (abs(H).^2 + mu) ;  xi = real(ifft2(X))
 *     we = W'(xi - z) ;  xw = s + we ;  bu = -we
 *     objective(outer+1) = 0.5 ||y - B xi||^2 + tau ||u||_1      (W xw = xi is the image estimate)
 * which is what runs (no division by mu).  Start xw by opts->initialization: 0 zeros, 2 W' B' y, 33333 xw_init; u = xw,
 * bu = 0, objective(1) from that state.  Stop rules 1, 2, 3 and the traces as SALSA_v2.m:442-482.
 * true_xw / xw_init / xw_out: [batch][3J+1][M*N] coefficients in the layout of sbtv_mrdwt_TI2D; x_out (optional): W xw_out.
 * objective / times / mses: [batch*(maxiter+1)], mses against true_xw over all coefficients; distance: [batch*maxiter] =
 * ||xw - u|| / sqrt(||xw||^2 + ||u||^2); numA = 1 + one per outer iteration, numAt = 1 (W' B' y), as SALSA_v2 counts them.
 * opts->TViters and the Chambolle knobs are ignored; opts->speculate bit 0: the host evaluates the stop rule one iteration
 * late while the next iteration already runs (the state is double-buffered: the result is that of the stopping iteration).
 * Images of a batch are solved one after another, image k bit for bit as alone.
 * Errors before any GPU work: those of the transforms; h not orthonormal (|sum h - sqrt 2| > 1e-10 or
 * |sum_k h[k] h[k+2m] - delta_m| > 1e-10) or mu[b] <= 0 -> SBTV_ERR_BADARG; odd pixel count -> SBTV_ERR_SIZE; stop criterion
 * and initialization as sbtv_SALSA_v2. */
int sbtv_SALSA_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                       const double *taps, int taille,
                       const double *h, int hlen, int levels,
                       const double *tau, const double *mu, const sbtv_salsa_opts *opts,
                       const double *true_xw, const double *xw_init,
                       double *xw_out, double *x_out,
                       double *objective, double *distance, double *times, double *mses,
                       int *numA, int *numAt, int *n_outer, int flags);
/* min over the IMAGE x  0.5 ||y - B x||^2 + tau ||W' x||_1  (the analysis-prior form; B: circular blur of `taps`), as
 * SALSA/SALSA_v2.m:389-494 solves it with its 'P' / 'PT' options (:98-101, 198-203): TVINITIALIZATION = 0, Psi = soft,
 * Phi = l1, A = B, AT = B', PT = W' = mrdwt_TI2D applied to the image (:389, 438), P = W = mirdwt_TI2D applied to the
 * coefficients (:434), and invLS(r) = real(ifft2(fft2(r) ./ (abs(H).^2 + mu))), the exact x-minimiser because W W' = I:
 *     start:  x by opts->initialization (0 zeros, 2 B'y, 33333 x_init) ;  PTx = W'x ;  u = PTx ;  bu = 0            (:367-393)
 *             objective(1) = 0.5 ||y - B x||^2 + tau ||u||_1 ;  mses(1) = ||x - true_x||^2 / (M N)                  (:399-415)
 *     outer:  u   = soft(PTx - bu, tau/mu)                                                                          (:431)
 *             x   = invLS(B'y + mu * W(u + bu))                                                                     (:434-436)
 *             PTx = W'x ;  bu = bu + (u - PTx)                                                                      (:438-440)
 *             objective(outer+1) = 0.5 ||y - B x||^2 + tau ||u||_1 ;  mses(outer+1) = ||x - true_x||^2 / (M N)      (:442-449)
 *             distance(outer)    = ||PTx - u|| / sqrt(||PTx||^2 + ||u||^2)                                          (:451)
 *             stop rules 1, 2, 3 from outer = 2 on (:453-482); rule 2 is ||x - xprev|| / ||x|| on the image
 * What runs keeps the coefficient state (s, bu), s = u + bu: z = W s, X = (conj(H) .* fft2(y) + mu * fft2(z)) ./ (abs(H).^2 + mu),
 * x = real(ifft2(X)), w = W'x, then one pass over the coefficients recovers u = s - bu (exactly zero where the threshold cut
 * it), takes the sums of the traces, forms bu + (u - w) and the next s = soft(w - bu, tau/mu) + bu.
 * true_x / x_init / x_out: [batch][M*N] images; x_out is required.  objective / times / mses: [batch*(maxiter+1)]; distance:
 * [batch*maxiter]; numA = 1 + one per outer iteration, numAt = 1 (B'y), as SALSA_v2 counts them (P and PT are not counted).
 * opts->TViters and the Chambolle knobs are ignored; opts->speculate bit 0 as for sbtv_SALSA_wavelet (x, s and bu are
 * double-buffered: the result is that of the stopping iteration).  Images of a batch are solved one after another, image k bit
 * for bit as alone.  SBTV_DEVICE_PTRS applies to y / true_x / x_init / x_out.
 * Errors before any GPU work: those of sbtv_SALSA_wavelet, with its codes: h not orthonormal, mu[b] <= 0, tau / mu / x_out
 * NULL -> SBTV_ERR_BADARG; odd pixel count or tap reach >= min(M, N) -> SBTV_ERR_SIZE; stop criterion, initialization,
 * maxiter and PSF fit as sbtv_SALSA_v2. */
int sbtv_SALSA_analysis(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                        const double *taps, int taille,
                        const double *h, int hlen, int levels,
                        const double *tau, const double *mu, const sbtv_salsa_opts *opts,
                        const double *true_x, const double *x_init, double *x_out,
                        double *objective, double *distance, double *times, double *mses,
                        int *numA, int *numAt, int *n_outer, int flags);
/* min over the IMAGE x  0.5 * sum( m .* (B x - y).^2 ) + tau ||W' x||_1: the masked-observation likelihood of sbtv_SALSA_masked
 * (unknown boundaries, missing or weighted pixels) with the analysis prior of sbtv_SALSA_analysis.  No entry of the reference:
 * the mask-decoupling ADMM of Almeida & Figueiredo (IEEE TIP 2013), which states it for frame-analysis priors as for TV.
 * B: the circular blur of `taps`; m = mask: non-negative weights like y (0 = not observed), exactly as for sbtv_SALSA_masked (y
 * enters only as m .* y, its values under m = 0 must be finite); W' = mrdwt_TI2D, W = mirdwt_TI2D with an orthonormal h
 * (W W' = I).  The splits are u = W'x (coefficients) and v = B x (pixels), the scaled multipliers bu, bv follow SALSA_v2's
 * sign convention (SALSA/SALSA_v2.m:429-440):
 *     start:  x by opts->initialization (0 zeros, 2 B'(m .* y), 33333 x_init)
 *             Bx = B x ;  PTx = W'x ;  u = PTx ;  bu = 0 ;  v = Bx ;  bv = 0
 *             objective(1) = 0.5 sum(m .* (Bx - y).^2) + tau ||u||_1 ;  mses(1) = ||x - true_x||^2 / (M N)
 *     outer:  u   = soft(PTx - bu, tau/mu1)
 *             v   = (m .* y + mu2 * (Bx - bv)) ./ (m + mu2)
 *             X   = (mu1 * fft2(W(u + bu)) + mu2 * conj(H) .* fft2(v + bv)) ./ (mu1 + mu2 * abs(H).^2)
 *             x   = real(ifft2(X)) ;  Bx = real(ifft2(H .* X)) ;  PTx = W'x
 *             bu  = bu + (u - PTx) ;  bv = bv + (v - Bx)
 *             objective(outer+1) = 0.5 sum(m .* (Bx - y).^2) + tau ||u||_1 ;  mses(outer+1) = ||x - true_x||^2 / (M N)
 *             distance(outer, :) = ||PTx - u|| / sqrt(||PTx||^2 + ||u||^2),  ||Bx - v|| / sqrt(||Bx||^2 + ||v||^2)
 *             stop rules 1, 2, 3 of SALSA_v2.m:453-482 from outer = 2 on; rule 2 is ||x - xprev|| / ||x|| on the image
 * What runs keeps the coefficient state (s, bu), s = u + bu, as sbtv_SALSA_analysis does (u = s - bu is recovered by the one
 * pass over the coefficients), and the pixel state x, Bx, v, bv: z = W s, X = (conj(H) .* fft2(v + bv) + r * fft2(z)) ./
 * (abs(H).^2 + r) with r = mu1/mu2, then one pass over the pixels forms bv + (v - Bx), the next v and the sums of the traces.
 * true_x / x_init / x_out: [batch][M*N] images; x_out is required.  objective / times / mses: [batch*(maxiter+1)]; distance:
 * [batch*maxiter*2], entry (outer-1)*2 + {0,1}.  numA = 1 (the start's B x) + one per outer iteration (H .* X), numAt = one per
 * outer iteration (conj(H) .* fft2(v + bv)) + 1 when initialization = 2; P and PT are not counted.
 * mu2 decides the speed, not the answer.  opts->TViters and the Chambolle knobs are ignored; opts->speculate bit 0 as for
 * sbtv_SALSA_analysis (x, s and bu are double-buffered: the result is that of the stopping iteration).  Images of a batch are
 * solved one after another, image k bit for bit as alone.  SBTV_DEVICE_PTRS applies to y / mask / true_x / x_init / x_out.
 * Errors before any GPU work, with the codes of the two parents: mask, tau, mu1, mu2, x_out or h NULL, mu1[b] <= 0, mu2[b] <= 0,
 * h not orthonormal, levels < 2 -> SBTV_ERR_BADARG; odd pixel count or tap reach >= min(M, N) -> SBTV_ERR_SIZE; stop
 * criterion, initialization, maxiter and PSF fit as sbtv_SALSA_analysis.  With SBTV_HOST_PTRS a mask with a negative or
 * non-finite entry is rejected (SBTV_ERR_BADARG); a device-resident mask (it lives where y lives) is the caller's
 * responsibility, as for sbtv_SALSA_masked. */
int sbtv_SALSA_masked_analysis(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch,
                               const double *taps, int taille,
                               const double *h, int hlen, int levels,
                               const double *tau, const double *mu1, const double *mu2, const sbtv_salsa_opts *opts,
                               const double *true_x, const double *x_init, double *x_out,
                               double *objective, double *distance, double *times, double *mses,
                               int *numA, int *numAt, int *n_outer, int flags);
/* min over the IMAGE x  0.5 ||y - B x||^2 + tau1 TV(x) + tau2 ||W' x||_1: CoRAL (SALSA/CoRAL_v2.m:2-476) with the compound
 * regulariser it exists for, TV on the image plus l1 on the coefficients of the redundant wavelet frame.  In the reference's
 * terms P1 = P1' = identity with TVINITIALIZATION1 = 1, P2 = W = mirdwt_TI2D, P2' = W' = mrdwt_TI2D, Psi2 = soft, Phi2 = l1,
 * TVINITIALIZATION2 = 0, and invLS(r) = real(ifft2(fft2(r) ./ (abs(H).^2 + mu))), mu = mu1 + mu2 (:137), the exact
 * x-minimiser because W W' = I:
 *     start:  x by opts->initialization (0 zeros, 2 B'y, 33333 x_init) ;  u = x ;  bu = u ;  v = W'x ;  bv = v     (:349-361)
 *             objective(1) = 0.5 ||y - B x||^2 + tau1 TVnorm(u) + tau2 ||v||_1 ;  mses(1)                           (:366-382)
 *             pux = puy = 0
 *     outer:  u = chambolle_prox_TV_stop(x - bu, 'lambda', tau1/mu1, 'maxiter', TViters, 'dualvars', [pux puy])     (:401)
 *             v = soft(W'x - bv, tau2/mu2)                                                                          (:408)
 *             x = invLS(B'y + mu1 * (u + bu) + mu2 * W(v + bv))                                                     (:411-413)
 *             bu = bu + (u - x) ;  bv = bv + (v - W'x)                                                              (:417-421)
 *             objective(outer+1) = 0.5 ||y - B x||^2 + tau1 TVnorm(u) + tau2 ||v||_1 ;  mses(outer+1)               (:423-430)
 *             distance(outer, 1) = ||x - u|| / sqrt(||x||^2 + ||u||^2)                                              (:432)
 *             distance(outer, 2) = ||W'x - v|| / sqrt(||W'x||^2 + ||v||^2)                                          (:433)
 *             stop rules 1, 2, 3 from outer = 2 on (:435-466); rule 2 is ||x - xprev|| / ||x|| on the image
 * What runs keeps the pixel state x, u, bu, g1 = x - bu and the coefficient state (sv, bv), sv = v + bv, as
 * sbtv_SALSA_analysis does: z = W sv, s = (mu1 (u + bu) + mu2 z) / mu, X = (conj(H) .* fft2(y) + mu * fft2(s)) ./ (abs(H).^2 + mu),
 * x = real(ifft2(X)), w = W'x, then one pass over the coefficients recovers v = sv - bv (exactly zero where the threshold cut
 * it), takes its sums, forms bv + (v - w) and the next sv, and one pass over the pixels updates bu and forms the next prox
 * input.  The start is sv = bv = W'x: the first soft argument is exactly zero, as the first prox input is.
 * opts->TViters is the Chambolle count and the Chambolle knobs apply.  true_x / x_init / x_out: [batch][M*N] images; x_out is
 * required.  objective / times / mses: [batch*(maxiter+1)]; distance: [batch*maxiter*2], entry (outer-1)*2+{0,1}.
 * numA = 1 + one per outer iteration, numAt = 2 (B'y is formed twice, :189,219); P2 and P2' are not counted.
 * `speculate` as for sbtv_CoRAL_v2: bit 0 the host books an iteration one iteration late (x, sv and bv are double-buffered:
 * the result is that of the stopping iteration), bit 1 never launch the TV prox optimistically; the result is always that of
 * the exact Chambolle stop rule.  Images of a batch are solved one after another, image k bit for bit as alone; there is no
 * sharded variant.  SBTV_DEVICE_PTRS applies to y / true_x / x_init / x_out.
 * Errors before any GPU work, with the codes of sbtv_SALSA_analysis and sbtv_CoRAL_v2: h not orthonormal, tau1 / tau2 / mu1 /
 * mu2 / x_out NULL -> SBTV_ERR_BADARG; mu1[b] <= 0 or mu2[b] <= 0 -> SBTV_ERR_MISSING_LS; odd pixel count or tap reach >=
 * min(M, N) -> SBTV_ERR_SIZE; levels < 2 -> SBTV_ERR_BADARG; TViters <= 0 or maxiter < 1 -> SBTV_ERR_MAXITER; stop criterion,
 * initialization and PSF fit as sbtv_SALSA_v2. */
int sbtv_CoRAL_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                       const double *taps, int taille,
                       const double *h, int hlen, int levels,
                       const double *tau1, const double *tau2, const double *mu1, const double *mu2,
                       const sbtv_salsa_opts *opts,
                       const double *true_x, const double *x_init, double *x_out,
                       double *objective, double *distance, double *times, double *mses,
                       int *numA, int *numAt, int *n_outer, int flags);
/* min over the IMAGE x  ||W' x||_1  s.t.  ||B x - y||_2 <= epsilon: C-SALSA (SALSA/CSALSA_v2.m:160-561) with the wavelet analysis
 * prior, its 'P' / 'PT' mode (:111-114, 208-213, 402, 467-478, 492), for the caller who knows the noise level and not a
 * regularisation parameter.  In the reference's terms TVINITIALIZATION = 0, Psi = soft, A = B, AT = B', PT = W' = mrdwt_TI2D,
 * P = W = mirdwt_TI2D, and invLS(r, mu1) = real(ifft2(fft2(r) ./ (abs(H).^2 + mu1))) exactly as sbtv_CSALSA_v2 defines it.
 * That is the exact x-minimiser only for mu2 = 1; other mu2 run as the reference would run them with this handle.
 *     start:  x by opts->initialization (0 zeros, 2 B'y, 33333 x_init) ;  PTx = W'x ;  u = bu = 0 ;  v = bv = 0     (:378-408)
 *             epsilon = sqrt(M N + 8 sqrt(M N)) * sigma when epsilon[b] = 0 (or epsilon == NULL)                     (:413)
 *             criterion(1) = distance1(1) = ||B x - y|| ;  distance2(1) = ||PTx|| ;  mses(1)                         (:416-448)
 *     outer = 2..maxiter:
 *             x   = invLS(mu1 * W(u + bu) + mu2 * B'(y + v + bv), mu1) ;  PTx = W'x                                  (:467-473)
 *             u   = soft(PTx - bu, 1/mu1)                                                                            (:478)
 *             ve  = B x - y - bv ;  v = ve if ||ve|| <= epsilon, else ve / ||ve|| * epsilon                          (:481-489)
 *             bv  = bv - (B x - y - v) ;  bu = bu - (PTx - u)                                                        (:491-492)
 *             criterion(outer) = ||B x - y|| ;  distance1(outer) = ||B x - y - v|| ;  distance2(outer) = ||PTx - u|| (:494-497)
 *             mu1 *= continuationfactor ;  mu2 *= continuationfactor                                                 (:517-518)
 *             stop when the rule's value < tolA AND criterion(outer) <= epsilon; rules 1, 2, 3 (:521-541), rule 2 is
 *             ||x - xprev|| / ||x|| on the image
 * ONE DEVIATION: objective(outer) = ||W' x||_1, the objective of the problem, which stop rule 1 then uses.  The reference
 * records phi(x) with x the IMAGE (:423, 498), i.e. with its default Phi the l1 norm of the pixels, and probes a user's Phi
 * with coefficients (:357); this entry fixes Phi = ||W' .||_1.
 * What runs keeps the coefficient state (s, bu), s = u + bu, in one buffer each (only x is returned; x is double-buffered),
 * and by default the constraint split as the spectrum of ve and one scalar, as sbtv_CSALSA_v2 does.  A continuation factor
 * != 1, an image size whose FFT plan has no such row pass, or SBTV_CSALSA_SPECTRAL=0 keep v and bv as images.
 * Traces are 1-based like the reference: entry 0 is the state before the loop; every trace row has maxiter entries;
 * n_outer[b] = the last `outer`.  numA = 2 + one per iteration, numAt = 1 (+ 1 for initialization 2) + one per iteration, as
 * sbtv_CSALSA_v2 counts them; P and PT are not counted.  opts->TViters and the Chambolle knobs are ignored; opts->speculate bit 0:
 * the host evaluates the stop rule one iteration late (not with a continuation factor != 1); the result is the same.
 * true_x / x_init / x_out: [batch][M*N] images; x_out is required.  Images of a batch are solved one after another, image k
 * bit for bit as alone; there is no sharded variant.  SBTV_DEVICE_PTRS applies to y / true_x / x_init / x_out.
 * Errors before any GPU work, with the codes of sbtv_SALSA_analysis and sbtv_CSALSA_v2: h not orthonormal, levels < 2, mu1 /
 * mu2 / sigma / x_out NULL -> SBTV_ERR_BADARG; mu1[b] <= 0 or mu2[b] <= 0 -> SBTV_ERR_MISSING_LS; odd pixel count or tap
 * reach >= min(M, N) -> SBTV_ERR_SIZE; maxiter < 1 -> SBTV_ERR_MAXITER; stop criterion, initialization and PSF fit as
 * sbtv_SALSA_v2. */
int sbtv_CSALSA_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                        const double *taps, int taille,
                        const double *h, int hlen, int levels,
                        const double *mu1, const double *mu2, const double *sigma, const double *epsilon,
                        double continuationfactor, const sbtv_salsa_opts *opts,
                        const double *true_x, const double *x_init, double *x_out,
                        double *objective, double *distance1, double *distance2, double *criterion,
                        double *times, double *mses, int *numA, int *numAt, int *n_outer, int flags);

/* ---- empirical-Bayes estimate of theta for the wavelet-l1 prior (SALSA/run_deblur_synthesis_L1.m:125-156) -----------------
 * The script estimates the regularisation parameter before it solves the MAP problem: a MYULA chain on the wavelet
 * coefficients drives the log-scale stochastic update of SALSA/SAPG_algorithm_1.m:165-216, and the solve then runs at
 * tau = theta_EB sigma^2, mu = theta_EB (:167,175).  SAPG_algorithm_1.m as shipped cannot be called by that script: it wants
 * op.to_init, op.grad_t and a two-argument gradF for a second parameter `tau` that the script never defines (SURVEY.md
 * section 2.3).  This entry point is its theta part, which is what the script's comments and constants describe
 * (sbtv_SAPG_wavelet_semiblind below adds the tau part, with the PSF parameters as tau).
 * One chain per image y_b; state X: [3J+1][M*N] coefficients in the layout of sbtv_mrdwt_TI2D, dimX = (3J+1) M N; W =
 * mirdwt_TI2D, W' = mrdwt_TI2D, B = circular blur of taps[b], soft = SALSA/soft.m (the script's proxG, :137):
 *     X = xw0 (NULL: W' y, :153) ;  prox = soft(X, lambda theta(1))
 *     warm-up, ii = 2..warmup, theta fixed at th_init (SAPG_algorithm_1.m:131-141):
 *         X = X + gamma (prox - X)/lambda - gamma W'B'(B W X - y)/sigma2 + sqrt(2 gamma) Z ;  prox = soft(X, lambda th_init)
 *         logpi_wu(ii) = -||y - B W X||^2 / (2 sigma2) - th_init ||X||_1                   (logpi_wu(1) = 0)
 *     logpi(1) = logPi(X, theta(1)) ;  eta(1) = log th_init
 *     ii = 2..samples (:171-216):
 *         X = (same step) ;  prox = soft(X, lambda theta(ii-1)) ;  g = ||X||_1
 *         eta(ii) = clamp(eta(ii-1) + delta(ii) (dimX/theta(ii-1) - g) exp(eta(ii-1)), log min_th, log max_th)
 *         theta(ii) = exp(eta(ii)) ;  delta(i) = d_scale i^(-d_exp) / dimX                  (:111,180-182)
 *         gx(ii-1) = g ;  logpi(ii) = -||y - B W X||^2 / (2 sigma2) - theta(ii-1) g        (:190-191; gx(samples) = 0)
 *         tol_thetas(ii) = |m(ii) - m(ii-1)| / m(ii-1), m(i) = exp(mean(eta(burnIn..i)))    (:199-200; NaN while a window
 *             is empty, i.e. for 2 <= ii <= burnIn, like MATLAB's mean of an empty range; tol_thetas(1) = 0)
 *         mean_thetas(ii - burnIn) = m(ii) for ii > burnIn                                  (:209-211)
 *     theta_eb = exp(mean(eta(burnIn..samples)))                                            (:226)
 * op.stopTol is computed into tol_thetas but never breaks the loop (the shipped loop has no break either).  The means are
 * running sums in iteration order.
 * What runs: the prox is never stored.  One element-wise kernel per iteration recomputes soft(X, lambda theta) from X and the
 * theta the prox was formed with (theta(ii-2) in iteration ii, theta(1) at ii = 2), takes or draws the normals, reads X and
 * the gradient once, writes X once and leaves per-workgroup sums of |X|; a one-workgroup-per-chain kernel sums them in a
 * fixed order, steps eta / theta and writes the traces on the device, so the host enqueues iterations without waiting (one
 * synchronisation per 1024 iterations and at the end).  ||y - B W X||^2 of sample ii is the Parseval sum of the next
 * iteration's gradient pass; the last sample costs one extra synthesis + forward transform.  Chains of a batch share every
 * launch; every reduction is per chain and in a fixed order, so chain b is computed bit for bit as alone.
 *   noise: NULL (device Philox randn: pair q of chain b's coefficients in step s draws counter (q, s, chain_offset + b), steps
 *          count from 0 through the warm-up and on, as in sbtv_SAPG_algorithm) or host/device array of
 *          (max(warmup-1,0) + samples-1) * batch * dimX doubles, step-major, each step [batch][dimX] in the layout of X
 *   traces (host, may be NULL): thetas, gx, logpi, tol_thetas [batch*samples]; logpi_wu [batch*warmup];
 *          mean_thetas [batch*(samples-burnIn)];  theta_eb [batch] (required);  xw_last: last sample (may be NULL)
 *   SBTV_DEVICE_PTRS applies to y / xw0 / noise / xw_last.
 * Refused before any GPU work: what sbtv_SALSA_wavelet refuses for h / levels / size (non-orthonormal h -> SBTV_ERR_BADARG,
 * odd pixel count -> SBTV_ERR_SIZE); samples < 2, warmup < 0, burnIn < 1 or > samples, lambda / gamma / sigma2 <= 0, th_init
 * not within 0 < min_th <= th_init <= max_th, chain_offset < 0 -> SBTV_ERR_BADARG. */
typedef struct sbtv_sapg_wavelet_opts {
    int    samples;           /* op.samples                                              */
    int    warmup;            /* op.warmup; 0 and 1: no warm-up step                     */
    int    burnIn;            /* op.burnIn (1-based like the reference)                  */
    double lambda, gamma;     /* op.lambda, op.gamma (run_deblur_synthesis_L1.m:149-150) */
    double sigma2;            /* noise variance of the likelihood (:141-142)             */
    double th_init, min_th, max_th;
    double d_scale, d_exp;    /* delta(i) = d_scale * i^-d_exp / dimX                    */
    unsigned long long seed;  /* Philox seed when noise == NULL                          */
    int    chain_offset;      /* chain b draws the Philox stream chain_offset + b        */
} sbtv_sapg_wavelet_opts;
int sbtv_SAPG_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                      const double *taps, int taille,
                      const double *h, int hlen, int levels,
                      const sbtv_sapg_wavelet_opts *op, const double *xw0, const double *noise,
                      double *thetas, double *gx, double *logpi, double *logpi_wu,
                      double *mean_thetas, double *tol_thetas, double *theta_eb,
                      double *xw_last, int flags);

/* ---- semi-blind empirical Bayes for the wavelet-l1 prior: theta, the PSF parameters and sigma2 from one chain ------------
 * SALSA/SAPG_algorithm_1.m is a two-parameter algorithm: next to theta it carries `tau` with its own projected gradient step
 * (:105-108,117,133,149-151,174,185-186,204-205,213,236-242).  The script run_deblur_synthesis_L1.m never defines op.to_init,
 * op.grad_t or the two-argument gradF it needs; the TV half of this library defines exactly those closures for three PSF
 * families (dA/dp, the tap derivatives of sbtv_psf_taps).  This entry is SAPG_algorithm_1.m with tau = the PSF parameters p,
 * scaled as SAPG/SAPG_algorithm_laplace.m:172-178, plus the sigma2 step of SAPG_algorithm_laplace.m:181-186.  One chain per
 * image y_b; state, frame, soft, dimX = (3J+1) M N and the noise layout are those of sbtv_SAPG_wavelet; the blur is B_p, the
 * circular blur of sbtv_psf_taps(kind, psf_size, p): there is no `taps` argument.  P = M N, pm = p(ii-1), s = sigma2(ii-1):
 *     X = xw0 (NULL: W' y) ;  prox = soft(X, lambda theta(1))
 *     warm-up, ii = 2..warmup, at th_init, p_init, sigma2(1)  (SAPG_algorithm_1.m:131-141 with gradF(X, fix_tau)):
 *         the step below ;  logpi_wu(ii) = -||y - B_p W X||^2 / (2 sigma2(1)) - th_init ||X||_1       (logpi_wu(1) = 0)
 *     logpi(1) = logPi(X, theta(1), p(1), sigma2(1)) ;  eta(1) = log th_init ;  p(1) = p_init ;  sigma2(1) = op.sigma2
 *     ii = 2..samples:
 *         X    = ((X + gamma (prox - X)/lambda) - gamma (W'B_pm'(B_pm W X - y)/s)) + sqrt(2 gamma) Z               (:174)
 *         prox = soft(X, lambda theta(ii-1)) ;  g = ||X||_1                                                         (:175)
 *         eta(ii), theta(ii): exactly the log-scale step and clamp of sbtv_SAPG_wavelet                             (:180-182)
 *         r = B_pm W X - y ;  R = ||r||^2
 *         G_pq = <(dB/dp_q)(pm) W X, r> / s                                              (the script's missing op.grad_t)
 *         p_q(ii) = clamp(fix_p[q] ? p_true[q] : p_q(ii-1) - c_p[q] delta(ii) G_pq, p_min[q], p_max[q])            (:185-186)
 *         G_s = R/(2 s^2) - P/(2 s) ;  sigma2(ii) = clamp(fix_sigma ? sigma2(1) : s + c_sigma delta(ii) G_s, sigma2_min,
 *             sigma2_max)                                                           (SAPG_algorithm_laplace.m:181-186)
 *         logpi(ii) = -R/(2 s) - theta(ii-1) g ;  gx(ii-1) = g                                                      (:190-191)
 *         tol_thetas / mean_thetas as sbtv_SAPG_wavelet ;  tol_ps(q, ii) = |a(ii) - a(ii-1)| / a(ii-1) and
 *         mean_ps(q, ii - burnIn) = a(ii) with the ARITHMETIC mean a(i) = mean(p_q(burnIn..i))                (:204-205,213)
 *     theta_EB = exp(mean eta(burnIn..samples)) ;  p_EB, sigma2_EB = arithmetic means over burnIn..samples        (:226,236)
 *   delta(i) = d_scale i^(-d_exp) / dimX with dimX the COEFFICIENT count (:111); G_s uses the PIXEL count P, the dimension of
 *   y.  The clamps apply to fixed values too, as in sbtv_SAPG_algorithm: give bounds that contain p_true / sigma2.  A fixed
 *   PSF parameter starts at p_init like a free one and is p_true from ii = 2 on.  Laplace has one parameter: slot 1 of ps is
 *   p_init[1] throughout (as is p1_EB), slot 1 of grads, tol_ps and mean_ps stays 0.  The means are running sums in
 *   iteration order; an entry whose window is empty, or whose previous mean is 0, is NaN as in MATLAB.
 *   Deliberate deviation: SAPG_algorithm_1.m:190 evaluates logPi at the unclamped new `to`; that would cost another operator
 *   evaluation and is not what the TV family does (SAPG_algorithm_laplace.m:194).  logpi(ii) uses p(ii-1).
 *   Moffat alpha: utils/diff_moffat_alpha.m:17 (and with it the d0 of sbtv_psf_taps, which reproduces the reference) carries
 *   alpha/(2 pi) where the derivative of alpha^2/(2 pi) gives alpha/pi: half the derivative of psf_moffat.m, in every tap.  G_p
 *   of this entry is the derivative of ||y - B_p W X||^2 / (2 sigma2) (checked against a finite difference), so the Moffat
 *   G_p0 is twice the <d0-blur W X, r> / s of the TV family's closure: c_p[0] here corresponds to 2 c_alpha there.
 * What runs: device-resident like sbtv_SAPG_wavelet; the host enqueues without waiting, one
 * synchronisation per 1024 iterations and one at the end.  One iteration: row pass OP_GRADF on the column spectrum of W X
 * that the previous iteration left, inverse column pass, J analysis launches; the step kernel (the shared step function of
 * sbtv_SAPG_wavelet, sigma2 and the lagging theta read from device memory); J synthesis launches, forward column pass, a row
 * pass without store that leaves R and the two <dB W X, r> sums, so the residual of sample ii is known in iteration ii; the
 * update kernel, one workgroup per chain, every sum in a fixed order, which with a free PSF parameter also builds the taps
 * and derivative taps of p(ii) (MATLAB's column-major summation order); then the tap spectra.  With every PSF parameter fixed
 * at p_true = p_init no taps are computed on the device and no spectrum is rebuilt; the start spectra come from host taps
 * (sbtv_psf_taps).  Chains of a batch share every launch; chain b is computed bit for bit as alone.  There is no host-loop
 * variant, no lanes, no graph capture, no sharded variant and no reduce_fn.  PSF sizes other than 7 x 7 are accepted as far
 * as sbtv_SAPG_algorithm accepts them but are untested in this entry.
 *   p_start: NULL (every chain starts at op->p_init) or [batch*2], host: the start values of chain b
 *   noise: as sbtv_SAPG_wavelet, the same Philox counters
 *   traces (host, may be NULL): thetas, sigmas, gx, logpi, tol_thetas [batch*samples]; ps, tol_ps [batch*2*samples];
 *          grads (G_p0, G_p1, G_s) [batch*3*samples]; logpi_wu [batch*warmup]; mean_thetas [batch*(samples-burnIn)];
 *          mean_ps [batch*2*(samples-burnIn)];  eb (theta, p0, p1, sigma2) [batch*4] (required);  xw_last: last sample
 *   SBTV_DEVICE_PTRS applies to y / xw0 / noise / xw_last.
 * Refused before any GPU work: everything sbtv_SAPG_wavelet refuses, with its codes (op->sigma2 is sigma2(1)); kind or
 * psf_size as sbtv_SAPG_algorithm refuses them (SBTV_ERR_PSF); with SBTV_ERR_BADARG: a free PSF parameter without
 * 0 < p_min <= p_init <= p_max (every chain's start), c_p or c_sigma negative or non-finite, a free sigma2 without
 * 0 < sigma2_min <= sigma2 <= sigma2_max. */
typedef struct sbtv_sapg_wavelet_sb_opts {
    int    samples, warmup, burnIn;      /* as sbtv_sapg_wavelet_opts                    */
    double lambda, gamma;
    double sigma2;            /* sigma2(1); the noise variance throughout if fix_sigma   */
    double th_init, min_th, max_th;
    double d_scale, d_exp;    /* delta(i) = d_scale * i^-d_exp / dimX                    */
    unsigned long long seed;  /* Philox seed when noise == NULL                          */
    int    chain_offset;      /* chain b draws the Philox stream chain_offset + b        */
    int    kind;              /* SBTV_PSF_*        (from here on: as sbtv_sapg_opts)     */
    int    psf_size;
    int    fix_p[2];
    int    fix_sigma;
    double phi;
    double p_init[2], p_min[2], p_max[2], p_true[2];
    double sigma2_min, sigma2_max;
    double c_p[2], c_sigma;
} sbtv_sapg_wavelet_sb_opts;
int sbtv_SAPG_wavelet_semiblind(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                                const double *h, int hlen, int levels,
                                const sbtv_sapg_wavelet_sb_opts *op, const double *p_start,
                                const double *xw0, const double *noise,
                                double *thetas, double *ps, double *sigmas, double *gx, double *logpi,
                                double *logpi_wu, double *grads, double *mean_thetas, double *tol_thetas,
                                double *mean_ps, double *tol_ps, double *eb,
                                double *xw_last, int flags);

/* ---- a-8: FISTA with the TV prox ----------------------------------------
 * Replaces my_fista(b,A,AT,tau,L,Phi,Psi,stopcriterion,tolerance,maxiters,true,verbose)
 * (SALSA/my_fista.m:5-56) with Psi = cold-start Chambolle(prox_iters) and Phi = TVnorm
 * (run_moffat_demo.m:181-182), and my_deblur_fista (SALSA/my_deblur_fista.m:5-68) when
 * zero_start = 1 and L = 1.  objective/mses: [batch*maxiters]; n_iter[batch]. */
int sbtv_fista_tv(sbtv_ctx *ctx, const double *b, int M, int N, int batch,
                  const double *taps, int taille, const double *tau, double L,
                  int prox_iters, int stopcriterion, double tolerance, int maxiters,
                  int zero_start, const double *true_x, double *x_out,
                  double *objective, double *mses, int *n_iter, int flags);

/* ---- FISTA on the wavelet-l1 problem --------------------------------------
 * Replaces my_fista_l1(b,h,tau,W,WT,stopcriterion,tolerance,maxiters,true,verbose) (SALSA/my_fista_l1.m:5-68), the FISTA the
 * SALSA toolbox compares its solver with: min over x  0.5 ||b - B W x||^2 + tau ||x||_1 on the coefficients x of the frame of
 * sbtv_mrdwt_TI2D, A = B W, AT = W' B' (:12-13).  The reference fixes L = 1 (:7) and starts at zero (:20-22, t(1) = 1); its
 * iteration k = 2..maxiters is (:34-66)
 *     x_old = x ;  t_old = t
 *     y = y - (1/L) AT(A(y) - b) ;  x = soft(y, tau/L)
 *     t = 0.5 (1 + sqrt(1 + 4 t_old^2)) ;  y = x + ((t_old - 1)/t) (x - x_old)
 *     objective(k) = 0.5 ||A(x) - b||^2 + tau sum|x| ;  mses(k) = ||x - true||^2 / numel(true)
 *     criterion: 1 |objective(k) - objective(k-1)| / objective(k) ; 2 ||x - x_old|| / sqrt(sum x^2) ; 3 objective(k)
 *     break if criterion < tolerance          (from k = 2 on)
 * with objective(1), mses(1) from the start (:27-29).  IEEE semantics of the criteria are kept: at x = 0 rule 2 is 0/0 = NaN,
 * which is never below the tolerance.
 * What runs: the momentum point y is never stored.  The coefficients x_{k-1}, x_{k-2} and their images zx = W x live in two
 * buffers each that swap roles; with c the factor (t_old - 1)/t of the iteration before (0 for k = 2) iteration k is
 *     zy = zx_{k-1} + c (zx_{k-1} - zx_{k-2})  (= W y) ;  g = W' B'(B zy - b)
 *     x_k = soft((x_{k-1} + c (x_{k-1} - x_{k-2})) - (1/L) g, tau/L) ;  zx_k = W x_k ;  ||B zx_k - b||^2 by Parseval
 * one synthesis per iteration instead of two: a momentum pass over the pixels, the FFT triple of the gradient, one analysis
 * (J launches), the step pass over the coefficients with the sums of the traces, one synthesis (J launches), the residual
 * passes and one reduction launch.  The host evaluates the stop rule one iteration late while the next iteration runs;
 * that iteration writes the buffers of x_{k-1}, so xw_out / x_out are those of the stopping iteration.  With
 * SBTV_FISTA_L1_NOLAG the host waits for every iteration (same result).
 * b: [batch][M*N]; taps [batch][taille^2]; h / hlen / levels and the coefficient layout [batch][3J+1][M*N] as for
 * sbtv_SALSA_wavelet; tau[batch] (host) >= 0; L > 0 (any L >= ||B||^2 converges).  xw_init NULL: the zero start of the
 * reference; otherwise (an extension) x = y = xw_init, t = 1, objective(1) from that state.  xw_out (required): the
 * coefficients of the stopping iteration; x_out (optional): W xw_out.  true_xw may be NULL: mses is then not written.
 * objective / times / mses: [batch][maxiters], host, any may be NULL; entry 0 is the state before the loop, entry k-1
 * iteration k of the reference; n_iter[b] is the last k run, entries from n_iter[b] on are not written; times[0] = 0, then
 * wall seconds since the loop started when the host books the iteration.  maxiters = 1 returns the start state.
 * Images of a batch are solved one after another, image k bit for bit as alone.  SBTV_DEVICE_PTRS applies to b / true_xw /
 * xw_init / xw_out / x_out.  The call counter advances by 2 + 3 (n_iter - 1) per image, the reference's `calls` (:15-18).
 * Refused before any GPU work: b, taps, h, tau or xw_out NULL, batch < 1, L not finite or <= 0, tolerance NaN, a tau[b]
 * negative or not finite -> SBTV_ERR_BADARG; stopcriterion outside 1..3 -> SBTV_ERR_STOPCRITERION 'Invalid stopping
 * criterion!' (:57); maxiters < 1 -> SBTV_ERR_MAXITER; taps that do not fit -> SBTV_ERR_PSF; for h / levels / size what
 * sbtv_SALSA_wavelet refuses, with its codes (non-orthonormal h -> SBTV_ERR_BADARG, tap reach >= min(M, N) or an odd pixel
 * count -> SBTV_ERR_SIZE). */
#define SBTV_FISTA_L1_NOLAG 2   /* sbtv_fista_l1 only: the host waits for iteration k's scalars before it enqueues k+1 */
int sbtv_fista_l1(sbtv_ctx *ctx, const double *b, int M, int N, int batch,
                  const double *taps, int taille, const double *h, int hlen, int levels,
                  const double *tau, double L, int stopcriterion, double tolerance, int maxiters,
                  const double *true_xw, const double *xw_init,
                  double *xw_out, double *x_out,
                  double *objective, double *times, double *mses, int *n_iter, int flags);

/* ---- a-5/a-6: SAPG (MYULA) parameter estimation ---------------------------
 * Replaces SAPG_algorithm_Guassian / _moffat / _laplace (SAPG/ directory) for `batch`
 * independent chains.  One chain = one image y_b with its own state.  */
typedef struct sbtv_sapg_opts {
    int    kind;              /* SBTV_PSF_*                                              */
    int    psf_size;          /* 7                                                       */
    int    samples;           /* op.samples  (total_iter)                                */
    int    warmup;            /* op.warmup                                               */
    int    burnIn;            /* op.burnIn (1-based like the reference)                  */
    int    chambolleit;       /* 25 (run_Gaussian_demo.m:188)                            */
    int    fix_p[2];          /* op.fix_w1/op.fix_w2 (alpha/beta, b)                     */
    int    fix_sigma;
    int    share_gradients;   /* 0: independent chains. 1: all chains sample one image and
                                 average their gradients (the reference's vestigial
                                 `for jj=1:1 ... mean(g_*)`, SAPG_algorithm_moffat.m:158-173) */
    double lambda, gamma;     /* c.lam*op.lambda, c.gam*op.gamma                         */
    double th_init, min_th, max_th;
    double p_init[2], p_min[2], p_max[2], p_true[2], phi;
    double sigma2_init, sigma2_min, sigma2_max, sigma2_true;
    double d_scale, d_exp;    /* delta(i) = d_scale * i^-d_exp / dimX                    */
    double c_theta, c_p[2], c_sigma;
    unsigned long long seed;  /* Philox seed when noise == NULL                          */
    int    chain_offset;      /* index of this call's first chain among ALL chains: chain b draws the
                                 Philox stream chain_offset + b, so chains spread over several processes
                                 (sbtv.dist.split_chains) never repeat a stream                     */
    int    iter_offset;       /* resume (no counterpart in the reference; SURVEY.md section 5 checkpoint / resume): SAPG
                                 iteration ii of this call is iteration ii + iter_offset of the chain, i.e. its step is
                                 delta(ii + iter_offset).  Continue a chain of S samples with x0 = its last sample,
                                 th_init / p_init / sigma2_init = its last values, warmup = 0, iter_offset = S - 1.  The
                                 Philox steps of a call always count from 0: give a resumed segment its own seed.
                                 0 = the reference's loop.                                          */
} sbtv_sapg_opts;

/*   y: M*N*batch;  x0: start images (NULL -> y, SAPG_algorithm_Guassian.m:10-12)
 *   noise: NULL (device Philox randn) or host/device array with
 *          (warmup-1 + samples-1) * batch * M*N doubles, step-major, consumed
 *          in the reference's order (warm-up first)
 *   traces (host, may be NULL): thetas, sigmas [batch*samples]; ps [batch*2*samples];
 *          logpi [batch*samples]; logpi_wu [batch*warmup]; gx [batch*samples]; grads [batch*4*samples]
 *   eb[batch*4] : theta_EB, p0_EB, p1_EB, sigma2_EB ;  x_last: last sample (may be NULL)
 *   reduce_fn: when share_gradients=1 and the chains are spread over several
 *          processes, called once per iteration with (user, buf, n = 6) to SUM buf[n]
 *          across processes in place (e.g. an RCCL all-reduce); may be NULL.
 *          buf = {sum G_theta, sum G_p0, sum G_p1, sum G_sigma, chains, failed ranks}: a rank whose iteration
 *          failed locally still calls reduce_fn (with failed = 1) before it returns its error, and every other
 *          rank then returns SBTV_ERR_PEER, so no rank is left waiting inside the collective.  Every rank must
 *          run at least one chain (batch >= 1).
 *   The loop itself (SAPG_algorithm_Guassian.m:98-248) is device-resident: the gradients G_theta, G_p, G_sigma
 *          (:165-188), the projected updates (:166-194), the PSF taps of the new parameters and the traces are
 *          computed by a one-workgroup kernel at the end of every iteration, so the host enqueues iterations without
 *          waiting for them (one synchronisation per 1024 iterations and at the end).  A host `reduce_fn` needs the
 *          scalars on the host and therefore selects the host-side loop (as does SBTV_SAPG_HOST_LOOP): identical
 *          arithmetic for theta / p / sigma; the PSF taps then come from the host's libm instead of the device's
 *          (differences in the last bit of exp / pow).  With SBTV_REDUCE_DEVICE `reduce_fn` must be an
 *          sbtv_allreduce_dev_fn: it is called once per iteration with the DEVICE address of the same 6 doubles and
 *          the library's stream and must enqueue an in-place SUM over the processes that is ordered after the work
 *          already in that stream and before work enqueued later (e.g. ncclAllReduce / torch.distributed.all_reduce
 *          on that stream); it must not wait for the GPU.  In that mode the host runs ahead of the device, so a rank whose
 *          iteration fails locally keeps calling reduce_fn once per remaining iteration with {0, 0, 0, 0, 0 chains,
 *          1 failed} before it returns its error; its peers latch the flag on the device and return SBTV_ERR_PEER at
 *          their next synchronisation (every 1024 iterations and at the end).  Only a failure of reduce_fn itself makes
 *          a rank return at once. */
typedef int (*sbtv_allreduce_fn)(void *user, double *buf, int n);
typedef int (*sbtv_allreduce_dev_fn)(void *user, double *dev_buf, int n, void *hip_stream);
int sbtv_SAPG_algorithm(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                        const sbtv_sapg_opts *op, const double *x0, const double *noise,
                        double *thetas, double *ps, double *sigmas, double *logpi,
                        double *logpi_wu, double *gx, double *grads, double *eb,
                        double *x_last, sbtv_allreduce_fn reduce_fn, void *reduce_user, int flags);

/* ---- posterior moments of the MYULA samples (no entry point of the reference: the `weldford` accumulator that
 * SAPG/SAPG_algorithm_Guassian.m:233-235,246,292-293 and run_Gaussian_demo.m:291-295 leave commented out, its class not
 * shipped) ----------------------------------------------------------------------------------------------------------
 * sbtv_SAPG_algorithm_moments / sbtv_myula_moments run exactly the chain of sbtv_SAPG_algorithm / sbtv_myula (no bit of
 * the traces, EB estimates, last sample or Philox counters changes) and also return the per-pixel posterior mean (the
 * MMSE image) and variance of the samples, accumulated on the device in Welford form while each sample is produced.
 *   Iterations: iteration 1 is the state the loop starts from - for SAPG the state after the warm-up (the X of ii = 1 of
 *     SAPG_algorithm_Guassian.m:98), for MYULA y; iteration ii is the sample X after the MYULA step of iteration ii.  SAPG
 *     runs ii = 2..samples, sbtv_myula ii = 2..samples-1 (SALSA/myula.m:13; its last iteration is max(1, samples-1)).
 *     Warm-up samples are never used.
 *   Selection: the iterations first, first + thin, ... up to the last iteration.  first = 0 means op->burnIn for SAPG
 *     (where the reference creates its accumulator, ii == op.burnIn) and 1 for MYULA.  thin >= 1.  thin < 1, first < 0 or
 *     first beyond the last iteration -> SBTV_ERR_BADARG before any GPU work.
 *   Outputs per chain: post_mean, post_var = M2 / (n-1) (the unbiased sample variance; all zeros for n = 1) and
 *     post_count = n, the number of samples used.  Layout [batch][M*N] (pooled: [1][M*N]), column-major like every image
 *     here; post_mean / post_var are device pointers with SBTV_DEVICE_PTRS, post_count [batch or 1] is always a host
 *     array.  post_mean is required, post_var and post_count may be NULL.
 *   pooled = 1: one moment set over all chains of the call, formed from the per-chain sets with Chan's pairwise
 *     combination in chain order 0, 1, 2, ... (a lane split does not change the bits).  Only for chains of ONE posterior:
 *     SAPG with share_gradients = 1, MYULA chains with the same y, taps, theta and sigma2; otherwise SBTV_ERR_BADARG.
 *   The two accumulators (mean and M2, 16 B per pixel each) cost 32 B of memory traffic per pixel and selected iteration;
 *   unselected iterations launch the plain kernels. */
typedef struct sbtv_moments_opts {
    int first;                /* first iteration used (0: burnIn for SAPG, 1 for MYULA)                */
    int thin;                 /* every thin-th iteration from `first` (>= 1)                           */
    int pooled;               /* 1: one set over all chains of the call                                */
} sbtv_moments_opts;
int sbtv_SAPG_algorithm_moments(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                                const sbtv_sapg_opts *op, const double *x0, const double *noise,
                                double *thetas, double *ps, double *sigmas, double *logpi,
                                double *logpi_wu, double *gx, double *grads, double *eb,
                                double *x_last, sbtv_allreduce_fn reduce_fn, void *reduce_user,
                                const sbtv_moments_opts *mo, double *post_mean, double *post_var,
                                long long *post_count, int flags);

/* Plain MYULA chain at fixed parameters: replaces  xMAP = myula(op, im)  (SALSA/myula.m:1-22) with the closures
 * of SALSA/run_deblur_tv.m:126,131:  proxG(x,lambda,theta) = chambolle_prox_TV_stop(x,'lambda',lambda*theta,
 * 'maxiter',chambolleit),  gradF(x) = AT(A x - y)/sigma2.  x starts at y; samples-2 steps
 *   x = (1 - gamma/lambda) x - gamma (gradF(x) - prox/lambda) + sqrt(2 gamma) z        (:16, no abs())
 * theta[batch], sigma2[batch] host arrays; noise: NULL (device Philox, stream chain_offset + b) or
 * (samples-2)*batch*M*N doubles, step-major.  x_out: the last sample of every chain. */
int sbtv_myula(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
               double lambda, double gamma, const double *theta, const double *sigma2, int samples,
               int chambolleit, unsigned long long seed, int chain_offset, const double *noise,
               double *x_out, int flags);
/* sbtv_myula with the posterior moments of its samples (see sbtv_SAPG_algorithm_moments above) */
int sbtv_myula_moments(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                       double lambda, double gamma, const double *theta, const double *sigma2, int samples,
                       int chambolleit, unsigned long long seed, int chain_offset, const double *noise,
                       double *x_out, const sbtv_moments_opts *mo, double *post_mean, double *post_var,
                       long long *post_count, int flags);

/* ---- wavelet-l1 posterior at a fixed theta: MYULA on the frame coefficients, MMSE image and pixel variance ---------------
 * No entry of the reference.  It is the warm-up loop of SALSA/SAPG_algorithm_1.m:131-141 with the closures of
 * SALSA/run_deblur_synthesis_L1.m:135-146 (proxG = soft, g = l1, gradF = W'B'(B W xw - y)/sigma2), run at the caller's theta:
 * what follows sbtv_SAPG_wavelet once theta_EB is known (that entry returns only its last sample, and its theta moves).
 * One chain per image y_b with its own theta[b] and sigma2[b] (host arrays: a batch may sweep theta, or give every image its
 * theta_EB and noise level); state X, W, W', B, soft and dimX as for sbtv_SAPG_wavelet:
 *     X(1) = xw0 (NULL: W' y)
 *     ii = 2..samples:
 *         G     = W'B'(B W X(ii-1) - y)
 *         X(ii) = ((X + gamma (soft(X, lambda theta_b) - X)/lambda) - gamma (G/sigma2_b)) + sqrt(2 gamma) Z,   X = X(ii-1)
 *     ii = 1..samples (no off-by-one):
 *         gx(ii)    = ||X(ii)||_1
 *         logpi(ii) = -||y - B W X(ii)||^2 / (2 sigma2_b) - theta_b gx(ii)
 * The step is the expression of sbtv_SAPG_wavelet's step, one shared device function: a warm-up of that entry at
 * th_init = theta gives the same bits.
 * What runs: one iteration is that of sbtv_SAPG_wavelet without its parameter update.  ||y - B W X(ii)||^2 is the Parseval
 * sum of iteration ii+1's gradient pass; the last sample costs one extra synthesis + forward transform.  Nothing is
 * reduced per iteration: the partial sums of up to 1024 iterations wait in a ring, and one launch turns them into trace
 * entries on the device, one workgroup per chain and iteration, every sum in a fixed order.  The host enqueues without
 * waiting: one synchronisation per 1024 iterations and one at the end.  Chains of a batch share every launch; chain b is
 * computed bit for bit as alone.  The call counter advances as in sbtv_SAPG_wavelet.  No lanes, no graph capture and no
 * sharded variant.
 *   noise: NULL (device Philox randn with the counters of sbtv_SAPG_wavelet: pair q of chain b in step s draws
 *          (q, s, chain_offset + b), s = ii - 2) or host/device array of (samples-1) * batch * dimX doubles, step-major, each
 *          step [batch][dimX] in the layout of X
 *   gx, logpi: [batch*samples], host, may be NULL;  xw_last: the last sample, may be NULL
 * Moments (mo != NULL), of the iterations 1..samples: selection (first = 0 means 1, thin >= 1; first, first + thin, ...),
 * outputs (var = M2/(n-1), zeros for n = 1; post_count = n, host) and pooled = 1 (Chan's combination in chain order; only
 * for chains with the same y, taps, theta and sigma2) as for sbtv_myula_moments.
 *   post_mean / post_var: IMAGE domain, [batch or 1][M*N]: mean and variance of W X(ii), the MMSE image and its pixel
 *          variance.  The image of sample ii exists inside the level-1 synthesis launch of iteration ii+1 (of the final
 *          residual pass for ii = samples); that launch accumulates it in Welford form on the value it stores: 32 B per
 *          pixel and selected iteration, no extra launch, no re-read.
 *   coef_mean / coef_var: COEFFICIENT domain, [batch or 1][dimX]: E[xw | y] and the marginal variance per coefficient,
 *          accumulated by the step kernel on X(ii) in registers: 32 B per coefficient and selected iteration.
 *   At least one of post_mean, coef_mean; post_var needs post_mean, coef_var needs coef_mean.  Unselected iterations
 *   launch the plain kernels, and no bit of the chain or its traces depends on what is accumulated.
 *   SBTV_DEVICE_PTRS applies to y / xw0 / noise / xw_last / post_mean / post_var / coef_mean / coef_var.
 * Refused before any GPU work: what sbtv_SAPG_wavelet refuses for taps / h / levels / size, with its codes; with
 * SBTV_ERR_BADARG: samples < 2, lambda or gamma <= 0, any theta[b] or sigma2[b] <= 0, non-finite values, chain_offset < 0,
 * theta == NULL, sigma2 == NULL, thin < 1, first < 0, first > samples, a moment output without what it needs (above), a
 * moment output with mo == NULL, pooled = 1 on chains of different posteriors. */
typedef struct sbtv_myula_wavelet_opts {
    int    samples;            /* >= 2: iteration 1 is the start state, samples-1 MYULA steps follow */
    double lambda, gamma;      /* as sbtv_sapg_wavelet_opts                                          */
    unsigned long long seed;   /* Philox seed when noise == NULL                                     */
    int    chain_offset;       /* chain b draws the Philox stream chain_offset + b                   */
} sbtv_myula_wavelet_opts;
int sbtv_myula_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                       const double *taps, int taille, const double *h, int hlen, int levels,
                       const sbtv_myula_wavelet_opts *op,
                       const double *theta, const double *sigma2,
                       const double *xw0, const double *noise,
                       double *gx, double *logpi,
                       double *xw_last,
                       const sbtv_moments_opts *mo,
                       double *post_mean, double *post_var, long long *post_count,
                       double *coef_mean, double *coef_var,
                       int flags);

/* ---- wavelet-l1 posterior at a fixed theta: SK-ROCK on the frame coefficients ------------------------------------------
 * No entry of the reference.  The explicit stabilised sampler of Pereyra, Vargas Mieles, Zygalakis, "Accelerating proximal
 * Markov chain Monte Carlo by using an explicit stabilised method", SIAM J. Imaging Sci. 2020, on the target of
 * sbtv_myula_wavelet (the same Moreau-Yosida-smoothed posterior, the same W, W', B, soft, dimX, theta_b, sigma2_b, lambda):
 * one step costs `stages` gradient evaluations and is stable for a step of about stages^2 (2 - 4 eta/3) / L where MYULA
 * allows about 1 / L, so that at equal gradient work the chain travels much further.  The drift is
 *     D(K) = (soft(K, lambda theta_b) - K)/lambda - G(K)/sigma2_b,    G(K) = W'B'(B W K - y)
 * Coefficients (sbtv_skrock_coefficients: host, double), s = stages >= 2, damping eta > 0, T_j / U_j the Chebyshev
 * polynomials of the first / second kind:
 *     w0 = 1 + eta/s^2;   T_0 = 1, T_1 = w0, T_j = 2 w0 T_{j-1} - T_{j-2};   T_s'(w0) = s U_{s-1}(w0)
 *     w1 = T_s(w0) / T_s'(w0)
 *     mu_1 = w1/w0,  nu_1 = s w1/2,  kappa_1 = s w1/w0
 *     j = 2..s:  mu_j = 2 w1 T_{j-1}/T_j,  nu_j = 2 w0 T_{j-1}/T_j,  kappa_j = 1 - nu_j
 *     l_s = (s - 0.5)^2 (2 - 4 eta/3) - 1.5
 * One step from X = X(ii-1) to X(ii), Z standard normal in the layout of X (the SAME Z three times), q = sqrt(2 delta):
 *     P   = X + (nu_1 q) Z
 *     K_1 = (X + (mu_1 delta) D(P)) + (kappa_1 q) Z,    K_0 = X
 *     j = 2..s:  K_j = ((mu_j delta) D(K_{j-1}) + nu_j K_{j-1}) + kappa_j K_{j-2}
 *     X(ii) = K_s
 * evaluated as grouped here, no floating-point contraction.  X(1) = xw0 (NULL: W' y).  Traces, ii = 1..samples, no lag:
 *     gx(ii)    = ||X(ii)||_1
 *     logpi(ii) = -||y - B W X(ii)||^2 / (2 sigma2_b) - theta_b gx(ii)
 * Stability: delta <= l_s / L, L = ||B||^2/sigma2 + 1/lambda (sbtv_skrock_max_step; ||B|| = 1 for a normalised non-negative
 * PSF, and the frame is tight).  The entry does not police delta, as sbtv_myula_wavelet does not police gamma.  A delta near
 * the bound biases the stiff directions of the target (their stationary variance shrinks); it is the caller's trade.
 * What runs: one step is s gradient passes (synthesis, FFT triple with OP_GRADF, analysis), each followed by one
 * element-wise stage kernel (32 B per coefficient; the first 24 B, the last 40 B: it also forms P of the next step), and one
 * residual pass (synthesis, forward transform, row pass) on X(ii), which gives logpi(ii) and is where the image moments of
 * sample ii are accumulated.  Two coefficient buffers and G.  Nothing is reduced per step: partial sums of up to 1024
 * samples wait in a ring; one launch turns them into trace entries, one workgroup per chain and sample, every sum in a
 * fixed order; one synchronisation per 1024 steps and one at the end.  Chains of a batch share every launch; chain b is
 * computed bit for bit as alone.  The call counter advances by batch for sample 1 and by (2 stages + 1) batch per step.
 * No lanes, no graph capture and no sharded variant.
 *   noise: NULL (device Philox randn with the counters of sbtv_myula_wavelet: sample ii draws step ii - 2, so a seed names the
 *          same normals in both samplers) or (samples-1) * batch * dimX doubles, step-major, as for sbtv_myula_wavelet
 *   theta, sigma2, xw0, gx, logpi, xw_last, the moments (mo, post_*, coef_*: of the samples 1..samples) and
 *   SBTV_DEVICE_PTRS: as for sbtv_myula_wavelet; no bit of the chain depends on what is accumulated.
 * Refused before any GPU work: what sbtv_myula_wavelet refuses (gamma aside), with its codes; with SBTV_ERR_BADARG also
 * stages < 2, delta <= 0, eta <= 0 and non-finite values. */
typedef struct sbtv_skrock_wavelet_opts {
    int    samples;            /* >= 2: sample 1 is the start state, samples-1 steps follow          */
    int    stages;             /* s >= 2 gradient evaluations per step                               */
    double lambda, delta, eta; /* Moreau-Yosida parameter, step (<= l_s/L), damping (e.g. 0.05)      */
    unsigned long long seed;   /* Philox seed when noise == NULL                                     */
    int    chain_offset;       /* chain b draws the Philox stream chain_offset + b                   */
} sbtv_skrock_wavelet_opts;
int sbtv_skrock_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch,
                        const double *taps, int taille, const double *h, int hlen, int levels,
                        const sbtv_skrock_wavelet_opts *op,
                        const double *theta, const double *sigma2,
                        const double *xw0, const double *noise,
                        double *gx, double *logpi,
                        double *xw_last,
                        const sbtv_moments_opts *mo,
                        double *post_mean, double *post_var, long long *post_count,
                        double *coef_mean, double *coef_var,
                        int flags);
/* Host only.  The table above: mu, nu, kappa [stages] (entry j-1 is stage j), omega[2] = {w0, w1}, ls = l_s; any output
 * may be NULL.  SBTV_ERR_BADARG: stages < 2, eta <= 0 or not finite. */
int sbtv_skrock_coefficients(int stages, double eta, double *mu, double *nu, double *kappa, double *omega, double *ls);
/* Host only.  delta_max = l_s / (normB2/sigma2 + 1/lambda), normB2 = ||B||^2.  SBTV_ERR_BADARG: stages < 2, eta, sigma2 or
 * lambda <= 0, normB2 < 0, non-finite values, delta_max == NULL. */
int sbtv_skrock_max_step(int stages, double eta, double sigma2, double lambda, double normB2, double *delta_max);

/* ---- TV posterior at fixed parameters: SK-ROCK in the image domain -------------------------------------------------------
 * No entry of the reference.  The sampler above on the target of sbtv_myula (the closures of SALSA/run_deblur_tv.m:126,131 with
 * theta[b] and sigma2[b] per chain), the experiment of the SK-ROCK paper itself.  The drift is
 *     D(K) = (prox(K) - K)/lambda - AT(A K - y)/sigma2_b,
 *     prox(K) = chambolle_prox_TV_stop(K, 'lambda', lambda theta_b, 'maxiter', chambolleit)   (the library's tol / tau)
 * and every evaluation of the prox starts from zero duals, as sbtv_myula's does.  Table and step: exactly those stated for
 * sbtv_skrock_wavelet above (P, K_1, K_j, the SAME Z three times, q = sqrt(2 delta)), grouped as written there, no
 * floating-point contraction; the table is sbtv_skrock_coefficients.  X(1) = x0 (NULL: y).  Samples ii = 2..samples, no
 * off-by-one: the samples-1 quirk of SALSA/myula.m:13 is NOT copied.  Traces, ii = 1..samples:
 *     gx(ii)    = TVnorm(X(ii))
 *     logpi(ii) = -||y - A X(ii)||^2 / (2 sigma2_b) - theta_b gx(ii)
 * Stability: delta <= sbtv_skrock_max_step(stages, eta, sigma2, lambda, 1.0, ...) (||A|| = 1 for a normalised non-negative
 * PSF; the prox term has Lipschitz constant 1/lambda).  The entry does not police delta, as sbtv_myula does not police gamma.
 * What runs: one step is s x (cold prox, gradient pass, one element-wise stage kernel: 32 B per pixel the first, 40 B a middle
 * one, 48 B the last, which also forms P of the next step) and, when a trace is requested, one residual pass on X(ii); the TV
 * partials ride on its forward column pass where the size allows.  Every stage kernel re-arms the prox control blocks, so no
 * reset launch sits inside a step.  Two image buffers, prox and gradient.  Partial sums of up to 1024 samples wait in a ring;
 * one launch turns them into trace entries, every sum in a fixed order; one synchronisation per 1024 steps and one at the
 * end.  With gx == NULL and logpi == NULL the residual pass is not launched.  Chains of a batch share every launch; chain b is
 * computed bit for bit as alone.  The call counter does not advance: the operator layer counts nothing for the s gradient
 * passes and the residual pass of a step, as for sbtv_myula.  No lanes, no graph capture, no sharded variant, and the stage is
 * not fused into the inverse column pass.
 *   noise: NULL (device Philox randn with the counters of sbtv_myula: pair q of chain b at sample ii draws
 *          (q, ii - 2, chain_offset + b), so a seed names the same normals in both samplers) or (samples-1) * batch * M*N
 *          doubles, step-major, host or device
 *   gx, logpi: [batch][samples], host, either may be NULL;  x_last: the last sample, may be NULL
 * Moments (mo != NULL), of the samples 1..samples: selection (first = 0 means 1), pooling (pooled = 1 only for chains with the
 * same y, taps, theta and sigma2), outputs and refusals as for sbtv_myula_moments; accumulated in the registers of the last
 * stage kernel, unselected samples launch the plain kernel.  No bit of the chain or the traces depends on what is
 * accumulated or on which traces are requested.
 *   SBTV_DEVICE_PTRS applies to y / x0 / noise / x_last / post_mean / post_var.
 * Refused before any GPU work: what sbtv_myula refuses, with its codes, gamma aside (SBTV_ERR_MAXITER for chambolleit <= 0,
 * SBTV_ERR_PSF, SBTV_ERR_SIZE for an odd pixel count); with SBTV_ERR_BADARG: samples < 2, stages < 2, non-finite or <= 0
 * lambda / delta / eta / theta[b] / sigma2[b], chain_offset < 0, op / theta / sigma2 == NULL, thin < 1, first < 0,
 * first > samples, mo without post_mean, pooled = 1 on chains of different posteriors, a moment output with mo == NULL. */
typedef struct sbtv_skrock_opts {
    int    samples;            /* >= 2: sample 1 is the start state, samples-1 steps follow */
    int    stages;             /* s >= 2 drift evaluations per step                          */
    int    chambolleit;        /* > 0: Chambolle iterations of every prox, cold start        */
    double lambda, delta, eta; /* Moreau-Yosida parameter, step, damping (e.g. 0.05)         */
    unsigned long long seed;   /* Philox seed when noise == NULL                             */
    int    chain_offset;       /* chain b draws the Philox stream chain_offset + b           */
} sbtv_skrock_opts;
int sbtv_skrock(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                const sbtv_skrock_opts *op, const double *theta, const double *sigma2,
                const double *x0, const double *noise, double *gx, double *logpi, double *x_last,
                const sbtv_moments_opts *mo, double *post_mean, double *post_var, long long *post_count, int flags);

/* ---- SAPG estimation of theta, the PSF parameters and sigma2 with SK-ROCK as its Markov kernel -------------------------------
 * No entry of the reference: sbtv_SAPG_algorithm with its MYULA move replaced by one step of sbtv_skrock, the authors' own
 * follow-up to MYULA-SAPG.  `batch` independent chains, one per image y_b.  The scalars, projections, traces and quirks are
 * exactly those of sbtv_SAPG_algorithm, and the arithmetic of the gradients and of the projected steps is the same code.  With
 * theta, p, s for theta(ii-1), p(ii-1), sigma2(ii-1):
 *     X = x0 (NULL: y)
 *     warm-up, ii = 2..warmup, at th_init, p_init, sigma2_init:
 *         X = SKROCK_step(X; th_init, p_init, sigma2_init);   logpi_wu(ii) = logPi(X, th_init, p_init, sigma2_init)
 *     logpi(1) = logPi(X, theta(1), p(1), sigma2(1))
 *     ii = 2..samples:
 *         X(ii) = SKROCK_step(X(ii-1); theta, p, s)
 *         r = A_p X(ii) - y;  R = ||r||^2;  g = TVnorm(X(ii))
 *         G_theta = dimX/theta - g;  G_pq = <dA/dp_q(p) X(ii), r>/s;  G_sigma = R/(2 s^2) - dimX/(2 s)
 *         theta(ii), p(ii), sigma2(ii): the projected steps of sbtv_SAPG_algorithm with
 *                                       delta(ii) = d_scale (ii + iter_offset)^(-d_exp)/dimX
 *         logpi(ii) = -R/(2 s) - theta g;   gx(ii-1) = g        (the index quirk of sbtv_SAPG_algorithm, kept)
 *     eb = means over burnIn..samples
 * SKROCK_step(X; theta, p, s) is the step of sbtv_skrock with delta = sk->dt: the table of sbtv_skrock_coefficients, P, K_1, K_j
 * and the SAME Z three times, grouped as written for sbtv_skrock_wavelet, no contraction, on the drift
 *     D(K) = (prox(K) - K)/lambda - A_p'(A_p K - y)/s,   prox(K) = chambolle_prox_TV_stop(K, lambda theta, maxiter = chambolleit)
 * from zero duals.  Two deliberate differences from the MYULA loop:
 *   - no abs() reflection of the new sample, as in sbtv_skrock;
 *   - no lagging prox: every stage evaluates its prox at theta(ii-1), where the MYULA loop moves with the prox it formed at
 *     the end of the previous iteration.
 * op->gamma is ignored.  dt is not policed: the safe bound is sbtv_skrock_max_step(stages, eta, min(sigma2_min, sigma2_max),
 * lambda, 1.0, ...), taken at the smallest sigma2 the chain may reach, because sigma2 moves.
 * What runs: one step is, with a free PSF parameter, the spectra of the taps the previous update left on the device; stages x
 * (cold prox, gradient pass with the current spectrum, one stage kernel of sbtv_skrock, which reads sigma2 and lambda theta
 * from the device); one gradient-sum pass on X(ii) (the TV partials ride on its forward column pass where the size allows;
 * its row pass stores nothing and has no inverse); and one update kernel, one workgroup per chain, which totals the chain's
 * sums in a fixed order, steps its parameters, books its traces and burn-in sums and builds the taps and derivative taps of
 * p(ii) (the device's libm; every mask size).  The host only enqueues: one synchronisation per 1024 steps and one at the
 * end.  Chains of a batch share every launch but the arithmetic of none: chain b is computed bit for bit as alone.  The call
 * counter does not advance.  Not offered: reduce_fn, a host-side loop, lanes, graph capture, a sharded variant.
 *   noise: NULL (device Philox randn with the counters of sbtv_SAPG_algorithm: pair q of chain b draws (q, step,
 *          chain_offset + b), steps count from 0 through the warm-up and on) or (max(warmup-1, 0) + samples-1) * batch * M*N
 *          doubles, step-major, host or device
 *   traces, eb, x_last: layouts as for sbtv_SAPG_algorithm
 *   Moments (mo != NULL; NULL: none), of the iterations 1..samples as for sbtv_SAPG_algorithm_moments (iteration 1 is the
 *          state after the warm-up; first = 0 means burnIn), accumulated in the registers of the last stage kernel; no bit of
 *          the chain or its traces depends on them.  pooled = 1 only with batch = 1: the chains estimate their own parameters.
 *   SBTV_DEVICE_PTRS applies to y / x0 / noise / x_last / post_mean / post_var.
 * Refused before any GPU work: everything sbtv_SAPG_algorithm refuses, with its codes; with SBTV_ERR_BADARG also
 * share_gradients != 0, sk == NULL, stages < 2, non-finite or <= 0 dt / eta, and the moment refusals of sbtv_skrock (thin < 1,
 * first < 0, first > samples, mo without post_mean, a moment output with mo == NULL, pooled = 1 with batch > 1). */
typedef struct sbtv_sapg_skrock_step {
    int    stages;             /* s >= 2 drift evaluations per step                          */
    double dt;                 /* the step of the chain (delta of sbtv_skrock)               */
    double eta;                /* damping (e.g. 0.05)                                        */
} sbtv_sapg_skrock_step;
int sbtv_SAPG_skrock(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const sbtv_sapg_opts *op,
                     const sbtv_sapg_skrock_step *sk, const double *x0, const double *noise,
                     double *thetas, double *ps, double *sigmas, double *logpi, double *logpi_wu, double *gx,
                     double *grads, double *eb, double *x_last,
                     const sbtv_moments_opts *mo, double *post_mean, double *post_var, long long *post_count, int flags);

/* ---- masked-observation MYULA and SAPG on the TV model -----------------------------------------------------------
 * No entry of the reference: the chains of sbtv_myula and sbtv_SAPG_algorithm on the likelihood of sbtv_SALSA_masked, an
 * observation that does not wrap round or that has missing or weighted pixels.  With m = mask (M*N*batch non-negative weights
 * like y, 0 = not observed), n_obs = the number of pixels of a chain with m > 0 and B_p the circular blur at the PSF
 * parameters p:
 *     p(y | x, p, s2) ~ s2^(-n_obs/2) exp( -R / (2 s2) ),   R = sum( m .* (B_p x - y).^2 )
 *     gradF(x)  = B_p' ( m .* (B_p x - y) ) / s2
 *     G_theta   = dimX / theta - TVnorm(X)                     (dimX = M*N, unchanged: the prior covers every pixel)
 *     G_p(q)    = sum( (dB/dp_q X) .* m .* (B_p X - y) ) / s2
 *     G_sigma   = R / (2 s2^2) - n_obs / (2 s2)
 *     logPi     = -R / (2 s2) - theta * TVnorm(X)
 * Everything else is the loop of sbtv_myula / sbtv_SAPG_algorithm line for line: the MYULA move (the reflecting abs() in SAPG,
 * none in myula), the prox the SAPG move uses (formed at the end of the previous iteration), the order of the updates, the
 * projections, delta(ii), the burn-in means, the traces with their layouts and index quirks, and the Philox counters.  With
 * m = 1 everywhere the model is that of those entries; the sums are then taken in space where they take them by Parseval, so
 * the traces agree to rounding, not bit for bit.
 * y enters only as m .* y: its values under m = 0 must be finite and influence no output, with one exception: sbtv_myula_masked
 * always, and sbtv_SAPG_masked with x0 == NULL, start from y as given.
 * The steps gamma the demos compute (1 / (Lf + 1/lambda), Lf = ||B||^2 / sigma2) hold for max(m) <= 1; larger weights raise
 * the Lipschitz constant of gradF by max(m) and are the caller's to account for.
 * What runs: the gradient's middle and the three sums are spatial.  One element-wise kernel writes
 * r = m .* (B x - y) and leaves per-workgroup partial sums of R, <dB/dp_1 X, r>, <dB/dp_2 X, r>, summed in a fixed order without
 * atomics; one kernel, one workgroup per chain, totals them, runs the parameter step of sbtv_SAPG_algorithm (the same code),
 * books the traces and builds the taps of p(ii).  B X, dB/dp_1 X, dB/dp_2 X come from one forward column pass (grads books
 * G_p whether or not p is free, as sbtv_SAPG_algorithm does).  With the PSF fixed the r of the sums is the next gradient's
 * input and no spectrum is rebuilt; with a free PSF parameter B X and r are formed again after the update, with the new
 * spectrum, from the column spectrum still held.  sbtv_myula_masked and the warm-up take two FFT round trips per iteration
 * (B X, B' r).  The loops are device-resident: the host only enqueues, one synchronisation per 1024 iterations and one at the
 * end.  Chains of a batch share every launch but the arithmetic of none: chain b is computed bit for bit as alone.  n_obs is
 * counted on the device once per call.  Not offered: reduce_fn, share_gradients, a host-side loop, lanes, graph capture, a
 * sharded variant.  The call counter does not advance.
 *
 * sbtv_myula_masked: sbtv_myula / sbtv_myula_moments (arguments, noise layout, Philox counters, iterations 1 = y, 2..samples-1).
 *   mo == NULL: no moments, and post_mean, post_var, post_count must be NULL; otherwise as for sbtv_myula_moments (first = 0
 *   means 1), pooled = 1 only with batch = 1 (the chains have their own masks).
 * sbtv_SAPG_masked: sbtv_SAPG_algorithm (op, x0, noise, traces, eb, x_last and their layouts); moments as for sbtv_SAPG_skrock
 *   (mo == NULL: none; first = 0 means burnIn; pooled = 1 only with batch = 1).
 * SBTV_DEVICE_PTRS applies to y / mask / x0 / noise / x_out / x_last / post_mean / post_var.
 * Refused before any GPU work: everything sbtv_myula / sbtv_SAPG_algorithm refuse, with their codes; with SBTV_ERR_BADARG also
 * mask == NULL, share_gradients != 0, a moment output with mo == NULL, pooled = 1 with batch > 1 and, with SBTV_HOST_PTRS, a
 * negative or non-finite mask entry or a chain whose mask has no positive entry.  A device-resident mask is the caller's
 * responsibility, as for sbtv_SALSA_masked. */
int sbtv_myula_masked(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch,
                      const double *taps, int taille, double lambda, double gamma, const double *theta,
                      const double *sigma2, int samples, int chambolleit, unsigned long long seed, int chain_offset,
                      const double *noise, double *x_out, const sbtv_moments_opts *mo, double *post_mean,
                      double *post_var, long long *post_count, int flags);
int sbtv_SAPG_masked(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch,
                     const sbtv_sapg_opts *op, const double *x0, const double *noise,
                     double *thetas, double *ps, double *sigmas, double *logpi, double *logpi_wu, double *gx,
                     double *grads, double *eb, double *x_last,
                     const sbtv_moments_opts *mo, double *post_mean, double *post_var, long long *post_count, int flags);

/* ---- a-9: largest eigenvalue of A'A by power iteration --------------------
 * Replaces max_eigenval(A,At,params,im_size,tol,max_iter,verbose)
 * (utils/max_eigenval_Gaussian_Moffat.m:1-27, max_eigenval_Laplace.m:1-28).
 * x0: start vector (the reference draws randn; MATLAB's stream is unpinned). */
int sbtv_max_eigenval(sbtv_ctx *ctx, const double *taps, int taille, const double *x0,
                      int M, int N, double tol, int max_iter, double *val, int *iters, int flags);

/* ---- a-10: metrics ----------------------------------------------------------
 * sbtv_PSNR: utils/PSNR.m:2-4 ; sbtv_MSE: utils/MSE.m:1-4 (dB). out[batch]. */
int sbtv_PSNR(sbtv_ctx *ctx, const double *x_true, const double *x, int M, int N, int batch, double *out, int flags);
int sbtv_MSE(sbtv_ctx *ctx, const double *x_true, const double *x, int M, int N, int batch, double *out, int flags);

/* ---- several GPUs behind ONE host process ---------------------------------------------
 * The reference's host is a single MATLAB process (run_Gaussian_demo.m:199 calls the SAPG loop, :229-242 SALSA_v2);
 * a group gives such a host all the GPUs of a node without a second process: one context and one host thread per
 * entry of `devices` (an ordinal may repeat: "virtual shards" on one GPU).  Items are dealt to the shards in
 * contiguous blocks (sbtv_group_shard_of); only min(n, n_items) shards take part in a call.  All pointers are HOST
 * pointers, laid out exactly as for the single-context entry points with batch = n_items.
 *   sbtv_fista_tv_sharded, sbtv_CSALSA_v2_sharded, sbtv_CoRAL_v2_sharded: independent images, no exchange
 *                                (SALSA/my_fista.m:5, SALSA/CSALSA_v2.m:160, SALSA/CoRAL_v2.m:2); arguments as for the
 *                                single-context entry points.
 *   sbtv_SALSA_v2_sharded        independent images: no exchange; image k is computed bit for bit as by sbtv_SALSA_v2.
 *   sbtv_SAPG_algorithm_sharded  op->share_gradients = 0: independent images / chains (chain i draws the Philox stream
 *                                op->chain_offset + i whatever the sharding).  share_gradients = 1: n_items MYULA chains
 *                                on ONE image y (SAPG_algorithm_moffat.m:143-173, `G = mean(g_*)`), the six gradient sums
 *                                added up across the shards once per iteration by an in-process, in-stream exchange
 *                                (pinned peer-visible slots + events; no GPU ever waits for its host, no RCCL).  A shard
 *                                that fails keeps the exchange in step until the end of the loop; the others return
 *                                SBTV_ERR_PEER and the call returns the failing shard's status (sbtv_group_last_error).
 */
typedef struct sbtv_group sbtv_group;
int         sbtv_group_create(const int *devices, int n, sbtv_group **out);
int         sbtv_group_destroy(sbtv_group *g);
int         sbtv_group_size(const sbtv_group *g);
sbtv_ctx   *sbtv_group_ctx(sbtv_group *g, int i);            /* context of shard i (e.g. for sbtv_last_timing) */
const char *sbtv_group_last_error(const sbtv_group *g);
/* which shard computes `item` of n_items, and that shard's block [first, first + count) */
int         sbtv_group_shard_of(const sbtv_group *g, int n_items, int item, int *shard, int *first, int *count);
int sbtv_SALSA_v2_sharded(sbtv_group *g, const double *y, int M, int N, int n_items,
                          const double *taps, int taille, const double *tau, const double *mu,
                          const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                          double *x_out, double *objective, double *distance, double *times, double *mses,
                          int *numA, int *numAt, int *n_outer);
/* device-resident variant: y[r] / true_x[r] / x_init[r] / x_out[r] (r < min(n, n_items)) are DEVICE pointers on shard r's
 * device to that shard's block of images (sbtv_group_shard_of: first, count), laid out as for sbtv_SALSA_v2 with
 * SBTV_DEVICE_PTRS; true_x and x_init may be NULL.  Nothing is copied between host and devices. */
int sbtv_SALSA_v2_sharded_dev(sbtv_group *g, const double *const *y, int M, int N, int n_items,
                              const double *taps, int taille, const double *tau, const double *mu,
                              const sbtv_salsa_opts *opts, const double *const *true_x,
                              const double *const *x_init, double *const *x_out, double *objective,
                              double *distance, double *times, double *mses, int *numA, int *numAt, int *n_outer);
int sbtv_SAPG_algorithm_sharded(sbtv_group *g, const double *y, int M, int N, int n_items,
                                const sbtv_sapg_opts *op, const double *x0, const double *noise,
                                double *thetas, double *ps, double *sigmas, double *logpi,
                                double *logpi_wu, double *gx, double *grads, double *eb, double *x_last);
int sbtv_fista_tv_sharded(sbtv_group *g, const double *b, int M, int N, int n_items,
                          const double *taps, int taille, const double *tau, double L,
                          int prox_iters, int stopcriterion, double tolerance, int maxiters,
                          int zero_start, const double *true_x, double *x_out,
                          double *objective, double *mses, int *n_iter);
int sbtv_CSALSA_v2_sharded(sbtv_group *g, const double *y, int M, int N, int n_items,
                           const double *taps, int taille, const double *mu1, const double *mu2,
                           const double *sigma, const double *epsilon, double continuationfactor,
                           const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                           double *x_out, double *objective, double *distance1, double *distance2,
                           double *criterion, double *times, double *mses,
                           int *numA, int *numAt, int *n_outer);
int sbtv_CoRAL_v2_sharded(sbtv_group *g, const double *y, int M, int N, int n_items,
                          const double *taps, int taille, const double *tau1, const double *tau2,
                          const double *mu1, const double *mu2, const double *mu_ls, int TViters2,
                          const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                          double *x_out, double *objective, double *distance, double *times, double *mses,
                          int *numA, int *numAt, int *n_outer);
/* independent images, no exchange; arguments as for sbtv_SALSA_masked, image k bit for bit as by that entry */
int sbtv_SALSA_masked_sharded(sbtv_group *g, const double *y, const double *mask, int M, int N, int n_items,
                              const double *taps, int taille, const double *tau, const double *mu1, const double *mu2,
                              const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                              double *x_out, double *objective, double *distance, double *times, double *mses,
                              int *numA, int *numAt, int *n_outer);

/* ---- diagnostics (no counterpart in the reference; SURVEY.md §5 sanitizer / tracing rows) ----
 * sbtv_diag_canary: with SBTV_CANARY=1 in the environment when the context was created, every device workspace of
 *   the context carries a 256-byte guard band on both sides and every entry point above ends by verifying all of
 *   them (SBTV_ERR_CANARY on damage).  This call verifies on demand: *enabled, number of guarded workspaces, damaged
 *   bytes.  poke = 1 first overwrites the rear guard of one workspace (self-test of the detector) and repairs it.
 * sbtv_diag_solve_stats: cumulative, this context and its lanes: out = {solves repeated with exact Chambolle launches because
 *   the stop rule (chambolle_prox_TV_stop.m:131) fired inside an optimistic prox, switches of a solve from subset error sums
 *   back to full sums, 0, 0}.
 * sbtv_diag_stage_stats: cumulative staging of large pageable host arrays by this context (and its lanes): out = {bytes
 *   host -> device, seconds, bytes device -> host, seconds}.  Arrays of >= 4 MB passed with SBTV_HOST_PTRS move through
 *   four copy lanes (pinned chunks, own streams, SBTV_STAGE_THREADS = 0..4); smaller ones through a plain hipMemcpyAsync.
 * sbtv_diag_prox_variant: which TV-prox kernel a (M, N, batch) problem takes: out = {columns per wave, waves per
 *   workgroup, waves per SIMD requested, rows per lane, tiles per image, 1 = temporally fused tile kernel / 0 = the
 *   one-iteration kernels (odd M, SBTV_SINGLE_STEP)} — lets a parity test assert which kernel it exercised.  (Value 2,
 *   the retired streaming pipeline kernel, is no longer returned.)
 * sbtv_diag_prox_geometry: the tile geometry behind that choice, from the same plan: out = {region rows, core rows, halo
 *   rows above the core, halo rows below, rows per lane, region columns, core columns, halo columns left, halo columns
 *   right, tile rows of the image, tile columns, 1 = the plan carries a workgroup -> tile table, first-round stagger in
 *   half-microseconds (0 = none), tile rows / tile columns of the one-iteration kernels, most iterations of one fused
 *   launch} — lets a test derive the image sizes that sit on a tile seam from the library instead of copying constants.
 * sbtv_diag_fft_plan: which FFT kernels an (M, N, batch) problem takes, from the host functions the launches themselves
 *   use: out = {1 = arbitrary-size (chirp-z) path, 1 = wave-granular kernels, column transform length n1, columns per
 *   column workgroup, threads per column workgroup, column workgroups per image, rows per row workgroup (0: the row pass
 *   is the point-wise operator), threads per row workgroup, row workgroups per image, row kernel kind (0 workgroup,
 *   1 software-pipelined, 2 point-wise), 1 = operator spectra tiled, Bluestein length for M, for N (0 off that path),
 *   values of l per thread of the tap-spectrum launch (`lch`), 1 = a shared-spectrum batch of this size folds into
 *   grid.x, bits: 1 = forward TV partials, 2 = the step / sub / skip_x column epilogues, 4 = OP_CSALSA available} -
 *   lets a test derive its sizes and assert which kernels it ran from the library instead of copied constants.
 * sbtv_diag_wavelet_geometry: the tile geometry of ONE level (1 .. levels - 1) of the wavelet frame kernels for an M x N
 *   image, a scaling filter of length hlen and `levels`, from the host functions and constants the launches of
 *   sbtv_mrdwt_TI2D / sbtv_mirdwt_TI2D themselves use; nothing is launched.  out = {J = levels - 1, stride s = 2^(level-1),
 *   run Q1 along dimension 1, Q2 along dimension 2, runs per stride s / Q1, s / Q2, outputs of a tile along dimension 1,
 *   along dimension 2 for analysis, along dimension 2 for synthesis, tiles along dimension 1, along dimension 2 for
 *   analysis, along dimension 2 for synthesis, halo samples (hlen - 1) Q1, (hlen - 1) Q2, static LDS bytes of the analysis
 *   kernel of this filter length, of the synthesis kernel}.  Refuses what the transforms refuse, with their codes
 *   (SBTV_ERR_BADARG: hlen not 2, 4, 6, 8 or levels < 2; SBTV_ERR_SIZE: (hlen - 1) 2^(levels - 2) >= min(M, N)), and a level
 *   outside 1 .. levels - 1 with SBTV_ERR_BADARG - lets a test derive the image sizes that sit on a tile seam, on a run cap
 *   or on a wrap of the halo from the library instead of copying constants.
 * sbtv_diag_spectral_pass: ONE forward-column, row, inverse-column triple of the solver loops on caller data (host
 *   pointers, column-major images), everything observable handed back; see sbtv_diag_pass.  Every refused argument is
 *   refused before the first launch, with the error the pass itself would give.
 * sbtv_diag_time_pass: times ONE pass of the hot path on scratch data of the given shape with HIP events on the
 *   context stream (`reps` launches after two untimed ones) -> average ms per launch and the algorithmic bytes of one
 *   launch.  pass: 0 forward column FFT of u+bu; 1 row pass with the SALSA spectral solve (forward FFT, operator,
 *   inverse FFT); 2 inverse column FFT fused with the SALSA bookkeeping; 3 plain inverse column FFT; 4 forward row
 *   FFT; 5 / 6 row pass with the SAPG gradient operators (with / without the PSF-parameter sums); 7 warm-started TV
 *   prox of 10 iterations incl. f (one SALSA outer iteration's share); 8 cold TV prox of 25 iterations incl. f;
 *   11..15 ONE fused Chambolle launch of 1..5 warm-started iterations without f and without control kernels (separates
 *   the fixed cost of a launch from the cost of an iteration).
 * sbtv_last_host_stats: how the HOST side of the most recent sbtv_SALSA_v2 or sbtv_fista_tv call waited for the device
 *   (the loop keeps one iteration queued ahead and polls completion tags in pinned memory): out = {waits, waits that found
 *   the scalars at the first look, waits that went past the spin window and slept, nanosleep calls, stream queries (the 50 ms
 *   fallback), seconds inside the waits, longest wait, seconds spent enqueueing, longest enqueue of one iteration,
 *   the outer iteration the longest wait was for, and what the operating system did to the calling thread during the
 *   loop (getrusage(RUSAGE_THREAD) deltas): voluntary / involuntary context switches, minor / major page faults}.
 * sbtv_diag_workspace: device address / capacity of a named internal workspace of the context, e.g. "salsa.u",
 *   "salsa.bu", "salsa.g": the state the most recent sbtv_SALSA_v2 call left behind (parity tests of intermediate arrays;
 *   with the default one-iteration lag they belong to the last iteration ENQUEUED, which is the stopping iteration
 *   only when the solve ran to MAXITERA).
 * sbtv_diag_switches: the SBTV_* environment switches that are set in this process, as "NAME=value ..." (returns their
 *   number; 0 and an empty string = the default kernels).  They are tuning / A-B hooks, read once per process. */
/* Layout helper for row-major hosts (NumPy, C; MATLAB needs none): dst[b][c][r] = src[b][r][c] for `batch` images of
 * rows x cols doubles - row-major images -> the column-major images every entry point takes, and back with rows / cols swapped. */
int sbtv_host_transpose(const double *src, double *dst, int batch, int rows, int cols);
int sbtv_diag_solve_stats(const sbtv_ctx *ctx, double out[4]);
int sbtv_diag_stage_stats(const sbtv_ctx *ctx, double out[4]);
int sbtv_diag_canary(sbtv_ctx *ctx, int poke, int *enabled, int *nbuf, int *nbad);
int sbtv_last_host_stats(const sbtv_ctx *ctx, double out[14]);
int sbtv_diag_workspace(sbtv_ctx *ctx, const char *name, void **dptr, size_t *bytes);
int sbtv_diag_switches(char *buf, size_t cap);
int sbtv_diag_time_pass(sbtv_ctx *ctx, int pass, int M, int N, int batch, int reps, double *ms_avg, double *alg_bytes);
int sbtv_diag_prox_variant(sbtv_ctx *ctx, int M, int N, int batch, int out[6]);
int sbtv_diag_prox_geometry(sbtv_ctx *ctx, int M, int N, int batch, int out[16]);
int sbtv_diag_fft_plan(sbtv_ctx *ctx, int M, int N, int batch, int out[16]);
int sbtv_diag_wavelet_geometry(sbtv_ctx *ctx, int M, int N, int hlen, int levels, int level, int out[16]);
/* op: the spectral operator of the row pass, 0 none, 1 X H, 2 X conj(H), 3 X / (|H|^2 + mu), 4 SALSA solve, 5 residual
 * sum only, 6 gradient with both PSF-parameter sums, 7 X |H|^2, 8 gradient, 9 C-SALSA solve with its state spectrum.
 * epilogue of the inverse column pass: 0 plain, 1 SALSA bookkeeping (bu in / out, g_out, sums; tru, xprev optional),
 * 2 ystep <- ystep - alpha x (x not stored), 3 g_out = x - sub_b, 4 bookkeeping that reads bu_in, writes bu and does not
 * store x; 2..4 only where the plan reports them.  shared_spec: taps / y / e0 hold ONE set for the whole batch, else one
 * per image.  repeats: the triple runs this many times, each on the x of the one before (epilogues that store x): two
 * passes of op 9 observe the state spectrum the first one left.  frozen (optional, per image): the image is skipped,
 * its outputs keep what the caller put there and its sums read 0.  acc [batch][3]: the row pass's sums; sums [batch][6]:
 * the bookkeeping sums; tv [batch] (optional): periodic TV of x from the forward column pass. */
typedef struct sbtv_diag_pass {
    int M, N, batch, op, epilogue, taille, shared_spec, repeats;
    const double *x, *add;
    const double *taps, *d1taps, *d2taps;
    const double *y, *e0;
    const double *mu, *cs;
    const int *frozen;
    const double *u, *bu_in, *tru, *xprev, *sub_b;
    double alpha;
    double *bu, *ystep;
    double *x_out, *g_out, *acc, *sums, *tv;
} sbtv_diag_pass;
int sbtv_diag_spectral_pass(sbtv_ctx *ctx, const sbtv_diag_pass *args);

#ifdef __cplusplus
}
#endif
#endif /* SBTV_H */

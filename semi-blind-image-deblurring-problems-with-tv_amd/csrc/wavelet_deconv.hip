// The three wavelet-l1 deconvolution solvers on the Parseval frame W of wavelet.hip:
//   sbtv_SALSA_wavelet   synthesis SALSA   min over xw  0.5 ||y - B W xw||^2 + tau ||xw||_1      (wavelet_one)
//   sbtv_SALSA_analysis  analysis SALSA    min over x   0.5 ||y - B x||^2    + tau ||W' x||_1    (analysis_one)
//   sbtv_fista_l1        FISTA on the synthesis problem (SALSA/my_fista_l1.m)                     (fista_l1_one)
// None of them calls the TV prox: an iteration is element-wise passes on the coefficients, the frame transforms and one pass
// of the blur operator, pipelined as the ADMM front-ends of admm.hip are (the host books an iteration's scalars one
// iteration late; the state is double-buffered, so the result of the stopping iteration is intact).  What the three share
// stands once: WavSolve (the set-up of a single-image solve, the booking of its traces, the tail of an iteration) and
// wav_batch (what an entry point does once its arguments are checked).  The images of a batch are solved one after another.
#include <chrono>
#include <cmath>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

#include "admm_run.inc"   // AB, ad_store_partials, AD_LOOP / AD_LD / AD_ST, ad_sub_kernel, ad_blocks, admm_common, upload_par, AdmmRun
#include "wav_step.inc"   // wav_init_kernel, wav_astep_kernel

// ---- wavelet-l1 SALSA (wavelet_one) -------------------------------------------------------------------------------
// The prox of an outer iteration on the state (s, we) of the previous one, xw = s + we and bu = -we:
//   u = soft(xw - bu, T) = soft(s + 2 we, T) ; s' = u + bu = u - we ; partials [2][nb]: |u|, u^2
__global__ __launch_bounds__(AB) void wav_prox_kernel(const double *__restrict__ s, const double *__restrict__ we,
                                                       double *__restrict__ sn, double T, double *__restrict__ partials,
                                                       size_t C) {
    double acc[2] = {0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 sv = AD_LD(s, q), wv = AD_LD(we, q);
        const double u0 = wav_soft(sv.x + 2.0 * wv.x, T), u1 = wav_soft(sv.y + 2.0 * wv.y, T);
        AD_ST(sn, q, make_double2(u0 - wv.x, u1 - wv.y));
        acc[0] += fabs(u0) + fabs(u1);
        acc[1] += u0 * u0 + u1 * u1;
    }
    ad_store_partials<2>(acc, partials);
}

// After the analysis we' = W'(xi - z) of an outer iteration: xw' = s' + we', u = s' + we (we: the previous iteration's), so
// xw' - u = we' - we.  partials [4][nb]: (xw'-u)^2, xw'^2, (xw'-true)^2, (xw'-xw)^2 with xw = s + we (sp == null: not summed)
__global__ __launch_bounds__(AB) void wav_post_kernel(const double *__restrict__ sn, const double *__restrict__ wn,
                                                       const double *__restrict__ we, const double *__restrict__ sp,
                                                       const double *__restrict__ tru, double *__restrict__ partials,
                                                       size_t C) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 sv = AD_LD(sn, q), wv = AD_LD(wn, q), wo = AD_LD(we, q);
        const double x0 = sv.x + wv.x, x1 = sv.y + wv.y;
        const double d0 = wv.x - wo.x, d1 = wv.y - wo.y;
        acc[0] += d0 * d0 + d1 * d1;
        acc[1] += x0 * x0 + x1 * x1;
        if (tru) {
            const double2 t = AD_LD(tru, q);
            const double m0 = x0 - t.x, m1 = x1 - t.y;
            acc[2] += m0 * m0 + m1 * m1;
        }
        if (sp) {
            const double2 so = AD_LD(sp, q);
            const double m0 = x0 - (so.x + wo.x), m1 = x1 - (so.y + wo.y);
            acc[3] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<4>(acc, partials);
}

// xw = s + we
__global__ __launch_bounds__(AB) void wav_sum_kernel(const double *__restrict__ s, const double *__restrict__ we,
                                                      double *__restrict__ xw, size_t C) {
    AD_LOOP(q, C) {
        const double2 sv = AD_LD(s, q), wv = AD_LD(we, q);
        AD_ST(xw, q, make_double2(sv.x + wv.x, sv.y + wv.y));
    }
}

// ---- analysis-prior wavelet SALSA (analysis_one) ------------------------------------------------------------------
// the pass itself, wav_astep_kernel, is in wav_step.inc
#include "ad_xsums.inc"   // ad_xsums_kernel: the image-domain sums of an outer iteration

// ---- wavelet-l1 FISTA (fista_l1_one) ------------------------------------------------------------------------------
// zy = zx + c (zx - zxo): the image W y of the momentum point y = x + c (x - xo), by linearity of W
__global__ __launch_bounds__(AB) void fl1_momentum_kernel(const double *__restrict__ zx, const double *__restrict__ zxo,
                                                           double c, double *__restrict__ zy, size_t P) {
    AD_LOOP(q, P) {
        const double2 a = AD_LD(zx, q), b = AD_LD(zxo, q);
        AD_ST(zy, q, make_double2(a.x + c * (a.x - b.x), a.y + c * (a.y - b.y)));
    }
}

// The step of an iteration (my_fista_l1.m:38-39,42 of the iteration before): y = x + c (x - xo) ; xn = soft(y - (1/L) g, T),
// T = tau / L, written over xo.  partials [3 or 4][nb]: |xn|, xn^2, (xn - x)^2 and, TRU, (xn - true)^2
template <bool TRU>
__global__ __launch_bounds__(AB) void fl1_step_kernel(const double *__restrict__ x, double *__restrict__ xo,
                                                       const double *__restrict__ g, const double *__restrict__ tru, double c,
                                                       double invL, double T, double *__restrict__ partials, size_t C) {
    constexpr int NQ = TRU ? 4 : 3;
    double acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = 0.0;
    AD_LOOP(q, C) {
        const double2 xv = AD_LD(x, q), ov = AD_LD(xo, q), gv = AD_LD(g, q);
        const double y0 = xv.x + c * (xv.x - ov.x), y1 = xv.y + c * (xv.y - ov.y);
        const double n0 = wav_soft(y0 - invL * gv.x, T), n1 = wav_soft(y1 - invL * gv.y, T);
        AD_ST(xo, q, make_double2(n0, n1));
        acc[0] += fabs(n0) + fabs(n1);
        acc[1] += n0 * n0 + n1 * n1;
        const double d0 = n0 - xv.x, d1 = n1 - xv.y;
        acc[2] += d0 * d0 + d1 * d1;
        if constexpr (TRU) {
            const double2 t = AD_LD(tru, q);
            const double m0 = n0 - t.x, m1 = n1 - t.y;
            acc[3] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<NQ>(acc, partials);
}

// ---- the scaffold of the three drivers ----------------------------------------------------------------------------
// the traces of one image that the three solvers have in common (each null: not wanted)
struct WavTraces {
    double *objective, *times, *mses;
};

// What a single-image solve opens, in this order: open (the operator layer "admm" and the sizes), the driver's own
// coefficient and image buffers (coef / image: each driver asks for those it uses, under the names they always had), arm (the
// scalars' workspaces and the AdmmRun).  In all three the coefficient pass leaves the l1 norm in sums[0] and the row pass the
// residual in sums[8], so the objective, the booking of the traces and the tail of an iteration stand here once.
struct WavSolve {
    sbtv_ctx *ctx = nullptr;
    BlurOp c;
    size_t P = 0, C = 0;                           // pixels, coefficients
    int nb = 0, nbp = 0, nrb = 0;                  // blocks of a coefficient pass, of a pixel pass, of the row pass
    double tau = 0.0, obj_prev = 0.0;
    const double *td = nullptr;                    // the true coefficients or image (null: no mses)
    WavTraces tr{};
    double *par = nullptr, *partials = nullptr, *sums = nullptr, *acc = nullptr;
    AdmmRun run;

    int open(sbtv_ctx *ctx_, const double *yd, int M, int N, const double *taps, int taille, const WavPlan &wp, double tau_,
             const double *td_, const WavTraces &tr_) {
        ctx = ctx_;
        tau = tau_;
        td = td_;
        tr = tr_;
        SBTV_TRY(admm_common(ctx, M, N, taps, taille, yd, &c));
        P = c.P;
        C = P * wp.bands();
        nb = ad_blocks(C);
        nbp = ad_blocks(P);
        nrb = fft_rows_blocks(c.fp);
        return 0;
    }
    int coef(const char *name, double **p) { return ws_get_t(ctx, name, C, p); }
    int image(const char *name, double **p) { return ws_get_t(ctx, name, P, p); }
    // mu given: the SALSA drivers' "admm.par" = {mu}, on the device when this returns (FISTA has no such parameter)
    int arm(const double *mu, int *numA, int *numAt, int *n_outer) {
        if (mu) SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));
        SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * 1024, &partials));   // the driver says what they are, nb or nbp each
        SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));            // [0] the l1 norm, [1..7] the driver's, [8] resid2
        SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));
        SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
        if (mu) SBTV_TRY(upload_par(ctx, par, {*mu, 0.0, 0.0, 0.0}));
        return 0;
    }
    double objective(const double *hs) const { return 0.5 * (hs[8] * c.parseval) + tau * hs[0]; }
    // entry i of the traces from the sums hs of its iterate (mses: hs[mse_slot] over n elements); entry 0 is the state before
    // the loop.  Returns the objective
    double book(int i, const double *hs, int mse_slot, size_t n) {
        const double f = objective(hs);
        if (tr.objective) tr.objective[i] = f;
        if (tr.mses && td) tr.mses[i] = hs[mse_slot] / (double)n;
        if (tr.times) tr.times[i] = i ? run.seconds() : 0.0;
        return f;
    }
    // the state before the loop, once the caller has enqueued its passes and added their jobs: the residual's job, the
    // reduction, the first 16 sums and entry 0 of the traces
    int book_start(RedJobs &jb, int mse_slot, size_t n) {
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        SBTV_HIP(ctx, hipGetLastError());
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        obj_prev = book(0, hs, mse_slot, n);
        return 0;
    }
    // tail of enqueue(k), after the jobs of the caller's partials: the residual's job, one reduction launch, 12 sums published
    int reduce_and_publish(int k, RedJobs &jb) {
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        return run.publish(k, sums, 12, 0);
    }
    // host side of iteration `outer` of the two SALSA drivers: traces and the stop rule of SALSA_v2.m:442-482.  mses is sums[4]
    // over n elements, stop rule 2 divides sums[5] by sums[den_slot]
    int salsa_process(int outer, const sbtv_salsa_opts *opts, size_t n, int den_slot, double *distance, bool *stop) {
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        run.numA += 1;                                                   // :443
        ctx->calls += 2;                                                 // invLS, A
        const double f = book(outer, hsl, 4, n);                         // :444, :446-449
        if (distance) distance[outer - 1] = sqrt(hsl[2]) / sqrt(hsl[3] + hsl[1]);   // :451
        *stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[5], hsl[den_slot], opts->tolA);
        obj_prev = f;
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// Wavelet-l1 deconvolution in the synthesis form (SALSA/run_deblur_synthesis_L1.m:160-180):
//     min over xw   0.5 ||y - B W xw||^2 + tau ||xw||_1,
// W the Parseval frame of wavelet.hip (W W' = I), solved as SALSA_v2.m:389-494 does with Psi = soft, Phi = l1, A = B W,
// AT = W' B' and invLS(r) = (r - W' F W r) / mu, F = |H|^2 / (|H|^2 + mu) in the Fourier domain.  With W W' = I one outer
// iteration of that is exactly
//     u = soft(xw - bu, tau / mu) ; s = u + bu ; z = W s ;
//     X = (conj(H) fft2(y) + mu fft2(z)) / (|H|^2 + mu) ; xi = real(ifft2(X))      (the row pass OP_SALSA on z)
//     we = W'(xi - z) ; xw = s + we ; bu = -we
// with the image estimate W xw = xi and ||y - B xi||^2 from the row pass's Parseval sum.  The coefficient state is (s, we):
// the next prox input is s + 2 we.  Both and xi are double-buffered, so the result of the stopping iteration is intact when
// the host evaluates the stop rule one iteration late.  Per outer iteration: the prox pass, one synthesis (J launches), the
// FFT triple, the difference, one analysis (J launches), the sums pass and one reduction launch.
// partials: [0..1] prox sums, [2..5] post sums, nb each; sums: [0] |u|, [1] u^2, [2..5] post sums, [8] resid2
int wavelet_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, const WavPlan &wp, double tau,
                double mu, const sbtv_salsa_opts *opts, const double *td, const double *xwi, double *xw_out_dev,
                double *x_out_dev, double *objective, double *distance, double *times, double *mses, int *numA, int *numAt,
                int *n_outer) {
    WavSolve s;
    SBTV_TRY(s.open(ctx, yd, M, N, taps, taille, wp, tau, td, {objective, times, mses}));
    const size_t P = s.P, C = s.C;
    const int nb = s.nb;
    double *sbuf[2], *wbuf[2], *xibuf[2], *z, *d;
    SBTV_TRY(s.coef("wav.s0", &sbuf[0]));
    SBTV_TRY(s.coef("wav.s1", &sbuf[1]));
    SBTV_TRY(s.coef("wav.we0", &wbuf[0]));
    SBTV_TRY(s.coef("wav.we1", &wbuf[1]));
    SBTV_TRY(s.image("admm.x0", &xibuf[0]));
    SBTV_TRY(s.image("admm.x1", &xibuf[1]));
    SBTV_TRY(s.image("admm.u", &z));
    SBTV_TRY(s.image("admm.g", &d));
    SBTV_TRY(s.arm(&mu, numA, numAt, n_outer));
    double *const partials = s.partials;
    const double T = tau / mu;                                           // :394
    s.run.numAt = 1;                                                     // ATy (:288)
    ctx->calls += 2;                                                     // AT(y), invLS(ATy)
    // the start xw as the state (s, we) = (xw, 0): bu = -we = 0 (:367-393)
    double *s0 = sbuf[0];
    if (opts->initialization == 0) {
        SBTV_HIP(ctx, hipMemsetAsync(s0, 0, sizeof(double) * C, ctx->stream));
        ctx->calls += 1;
    } else if (opts->initialization == 2) {                              // xw = W' B' y
        SBTV_TRY(op_apply(ctx, s.c, OP_MUL_HC, yd, d));
        SBTV_TRY(wav_analysis(ctx, wp, d, s0, 1));
    } else {
        SBTV_HIP(ctx, hipMemcpyAsync(s0, xwi, sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
    }
    SBTV_HIP(ctx, hipMemsetAsync(wbuf[0], 0, sizeof(double) * C, ctx->stream));
    // initial objective (:399-401): resid = y - B W xw
    {
        SBTV_TRY(wav_synthesis(ctx, wp, s0, xibuf[0], 1));
        SBTV_TRY(op_resid(ctx, s.c, xibuf[0], s.acc));
        SBTV_HIP(ctx, hipMemsetAsync(s.sums, 0, sizeof(double) * 16, ctx->stream));
        hipLaunchKernelGGL(wav_init_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)s0, td, partials, C);
        RedJobs jb;
        jb.add(partials, 2, nb, s.sums);
        SBTV_TRY(s.book_start(jb, 1, C));                                // :414
        s.run.numA += 1;
        ctx->calls += 1;
    }
    SBTV_TRY(s.run.start());
    const int lag = (opts->speculate & 1) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {                               // :423
        const int o = outer & 1, p = o ^ 1;
        double *sn = sbuf[o], *wn = wbuf[o], *xi = xibuf[o];
        const double *sp = sbuf[p], *we = wbuf[p];
        hipLaunchKernelGGL(wav_prox_kernel, dim3(nb), dim3(AB), 0, ctx->stream, sp, we, sn, T, partials, C);      // :432
        SBTV_TRY(wav_synthesis(ctx, wp, sn, z, 1));
        SBTV_TRY(op_solve(ctx, s.c, z, nullptr, s.c.Ys, s.par, s.acc, xi));    // :434-436
        hipLaunchKernelGGL(ad_sub_kernel, dim3(s.nbp), dim3(AB), 0, ctx->stream, (const double *)xi, (const double *)z, d, P);
        SBTV_TRY(wav_analysis(ctx, wp, d, wn, 1));
        hipLaunchKernelGGL(wav_post_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)sn, (const double *)wn, we,
                           (opts->stopcriterion == 2) ? sp : (const double *)nullptr, td, partials + (size_t)2 * nb, C);
        RedJobs jb;
        jb.add(partials, 6, nb, s.sums);
        return s.reduce_and_publish(outer, jb);
    };
    bool stop = false;
    auto process = [&](int outer) { return s.salsa_process(outer, opts, C, 3, distance, &stop); };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, opts->maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    SBTV_TRY(s.run.finish(P, last, nullptr, nullptr));                   // the result: xw = s + we, and the image xi
    hipLaunchKernelGGL(wav_sum_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)sbuf[last & 1],
                       (const double *)wbuf[last & 1], xw_out_dev, C);
    SBTV_HIP(ctx, hipGetLastError());
    if (x_out_dev)
        SBTV_HIP(ctx, hipMemcpyAsync(x_out_dev, xibuf[last & 1], sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Wavelet-l1 deconvolution in the analysis form, the 'P' / 'PT' mode of SALSA_v2.m (:98-101, 198-203):
//     min over the image x   0.5 ||y - B x||^2 + tau ||W' x||_1,
// solved as SALSA_v2.m:389-494 does with Psi = soft, Phi = l1, A = B, AT = B', PT = W', P = W and invLS(r) =
// real(ifft2(fft2(r) ./ (|H|^2 + mu))), the exact x-minimiser because W W' = I.  One outer iteration k on the coefficient
// state (s, bu), s = u + bu:
//     z = W s_k ;  X = (conj(H) fft2(y) + mu fft2(z)) / (|H|^2 + mu) ;  x_k = real(ifft2(X))      (the row pass OP_SALSA on z)
//     w_k = W' x_k ;  the step pass (wav_astep_kernel): u_k = s_k - bu_{k-1}, its sums, bu_k, s_{k+1}
// with ||y - B x_k||^2 from the row pass's Parseval sum and the image-domain sums of x_k from a pixel pass, launched only when
// 'TRUE_X' or stop rule 2 ask for them.  s, bu and x are double-buffered, so the result of the stopping iteration is intact
// when the host evaluates the stop rule one iteration late.  Per outer iteration: one synthesis (J launches), the FFT triple,
// one analysis (J launches), the step pass, the pixel pass and one reduction launch.
// partials: [0..3] step sums, nb each, then [0..2] pixel sums, nbp each; sums: [0..3] step sums, [4..6] pixel sums, [8] resid2
int analysis_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, const WavPlan &wp, double tau,
                 double mu, const sbtv_salsa_opts *opts, const double *td, const double *xi, double *x_out_dev,
                 double *objective, double *distance, double *times, double *mses, int *numA, int *numAt, int *n_outer) {
    WavSolve s;
    SBTV_TRY(s.open(ctx, yd, M, N, taps, taille, wp, tau, td, {objective, times, mses}));
    const size_t P = s.P, C = s.C;
    const int nb = s.nb, nbp = s.nbp;
    double *sbuf[2], *bbuf[2], *xbuf[2], *w, *z;
    SBTV_TRY(s.coef("wav.s0", &sbuf[0]));
    SBTV_TRY(s.coef("wav.s1", &sbuf[1]));
    SBTV_TRY(s.coef("wav.we0", &bbuf[0]));
    SBTV_TRY(s.coef("wav.we1", &bbuf[1]));
    SBTV_TRY(s.coef("wav.w", &w));
    SBTV_TRY(s.image("admm.x0", &xbuf[0]));
    SBTV_TRY(s.image("admm.x1", &xbuf[1]));
    SBTV_TRY(s.image("admm.u", &z));
    SBTV_TRY(s.arm(&mu, numA, numAt, n_outer));
    double *const partials = s.partials, *const ppix = partials + (size_t)4 * nb;
    const double T = tau / mu;                                           // :394
    const bool rule2 = opts->stopcriterion == 2;
    s.run.numAt = 1;                                                     // ATy (:288)
    ctx->calls += 2;                                                     // AT(y), invLS(ATy)
    if (opts->initialization == 0) ctx->calls += 1;                      // AT(zeros) (:369)
    SBTV_TRY(op_init_x(ctx, s.c, opts->initialization, yd, xi, xbuf[0]));   // :367-381
    // PTx = W'x ; u = PTx ; bu = 0 (:389-393) and the initial objective (:399-401): the step pass on (s, bu) = (PTx, 0)
    {
        SBTV_TRY(wav_analysis(ctx, wp, xbuf[0], w, 1));
        SBTV_HIP(ctx, hipMemsetAsync(bbuf[1], 0, sizeof(double) * C, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(s.sums, 0, sizeof(double) * 16, ctx->stream));
        hipLaunchKernelGGL(wav_astep_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)w, (const double *)bbuf[1],
                           (const double *)w, bbuf[0], sbuf[0], T, partials, C);
        SBTV_TRY(op_resid(ctx, s.c, xbuf[0], s.acc));
        RedJobs jb;
        jb.add(partials, 4, nb, s.sums);
        if (td) {
            hipLaunchKernelGGL(ad_xsums_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)xbuf[0], td,
                               (const double *)nullptr, ppix, P);
            jb.add(ppix, 3, nbp, s.sums + 4);
        }
        SBTV_TRY(s.book_start(jb, 4, P));                                // :415
        s.run.numA += 1;
        ctx->calls += 1;
    }
    SBTV_TRY(s.run.start());
    const int lag = (opts->speculate & 1) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {                               // :423
        const int o = outer & 1, p = o ^ 1;
        double *xn = xbuf[o];
        SBTV_TRY(wav_synthesis(ctx, wp, sbuf[p], z, 1));                 // P(u + bu) (:434)
        SBTV_TRY(op_solve(ctx, s.c, z, nullptr, s.c.Ys, s.par, s.acc, xn));   // :434-436
        SBTV_TRY(wav_analysis(ctx, wp, xn, w, 1));                       // :438
        hipLaunchKernelGGL(wav_astep_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)sbuf[p],
                           (const double *)bbuf[p], (const double *)w, bbuf[o], sbuf[o], T, partials, C);   // :440, :431
        RedJobs jb;
        jb.add(partials, 4, nb, s.sums);
        if (td || rule2) {
            hipLaunchKernelGGL(ad_xsums_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)xn, td,
                               rule2 ? (const double *)xbuf[p] : (const double *)nullptr, ppix, P);
            jb.add(ppix, 3, nbp, s.sums + 4);
        }
        return s.reduce_and_publish(outer, jb);
    };
    bool stop = false;
    auto process = [&](int outer) { return s.salsa_process(outer, opts, P, 6, distance, &stop); };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, opts->maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return s.run.finish(P, last, xbuf[last & 1], x_out_dev);
}

// ------------------------------------------------------------------------------------------------
// FISTA on the same problem (SALSA/my_fista_l1.m:5-68): min over x  0.5 ||b - B W x||^2 + tau ||x||_1.  The reference's
// iteration k = 2..maxiters is (:34-47)
//     y = y - (1/L) W'B'(B W y - b) ; x = soft(y, tau/L) ; t = 0.5 (1 + sqrt(1 + 4 t_old^2)) ; y = x + ((t_old-1)/t)(x - x_old)
//     objective(k) = 0.5 ||B W x - b||^2 + tau sum|x|
// What runs keeps x_{k-1}, x_{k-2} and their images zx = W x in two buffers each and never stores y: with c the momentum
// factor of the iteration before (0 for k = 2; t and c depend on no data, the host knows them when it enqueues)
//     zy = zx_{k-1} + c (zx_{k-1} - zx_{k-2})              (= W y by linearity; fl1_momentum_kernel)
//     g  = W' B'(B zy - b)                                  (op_gradf, wav_analysis)
//     x_k = soft((x_{k-1} + c (x_{k-1} - x_{k-2})) - (1/L) g, tau/L)   over x_{k-2}, with its sums (fl1_step_kernel)
//     zx_k = W x_k over zx_{k-2} ; ||B zx_k - b||^2         (wav_synthesis, op_resid)
// one synthesis per iteration where the reference has two (W y inside A(y), W x for the objective).  The host books the
// traces and the stop rule one iteration late (lag 1); iteration k + 1 writes the buffers of x_{k-1}, so x_k and zx_k are
// intact when the rule of iteration k is seen.
// partials: [0..3] step sums, nb each; sums: [0] |x|, [1] x^2, [2] (x-xprev)^2, [3] (x-true)^2, [8] resid2
int fista_l1_one(sbtv_ctx *ctx, const double *bd, int M, int N, const double *taps, int taille, const WavPlan &wp, double tau,
                 double L, int stopcriterion, double tolerance, int maxiters, int lag, const double *td, const double *xwi,
                 double *xw_out_dev, double *x_out_dev, double *objective, double *times, double *mses, int *n_iter) {
    WavSolve s;
    SBTV_TRY(s.open(ctx, bd, M, N, taps, taille, wp, tau, td, {objective, times, mses}));
    const size_t P = s.P, C = s.C;
    const int nb = s.nb, nbp = s.nbp;
    double *xb[2], *zb[2], *zy, *gi, *g;
    SBTV_TRY(s.coef("wav.s0", &xb[0]));
    SBTV_TRY(s.coef("wav.s1", &xb[1]));
    SBTV_TRY(s.coef("wav.we0", &g));
    SBTV_TRY(s.image("admm.x0", &zb[0]));
    SBTV_TRY(s.image("admm.x1", &zb[1]));
    SBTV_TRY(s.image("admm.u", &zy));
    SBTV_TRY(s.image("admm.g", &gi));
    SBTV_TRY(s.arm(nullptr, nullptr, nullptr, n_iter));
    double *const partials = s.partials;
    const double T = tau / L, invL = 1.0 / L;                            // :38-39
    const int nq = td ? 4 : 3;
    ctx->calls += 2;                                                     // AT(b) (:20), A(x) (:28)
    // iterate 1, the start (:20-22; x = y = xw_init): in the buffers of parity 1, and as "x_0" in those of parity 0, where
    // c = 0 multiplies a zero difference
    if (xwi) {
        SBTV_HIP(ctx, hipMemcpyAsync(xb[1], xwi, sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(xb[0], xwi, sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        SBTV_HIP(ctx, hipMemsetAsync(xb[1], 0, sizeof(double) * C, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(xb[0], 0, sizeof(double) * C, ctx->stream));
    }
    {
        SBTV_TRY(wav_synthesis(ctx, wp, xb[1], zb[1], 1));               // :27-29
        SBTV_HIP(ctx, hipMemcpyAsync(zb[0], zb[1], sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
        SBTV_TRY(op_resid(ctx, s.c, zb[1], s.acc));
        SBTV_HIP(ctx, hipMemsetAsync(s.sums, 0, sizeof(double) * 16, ctx->stream));
        hipLaunchKernelGGL(wav_init_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)xb[1], td, partials, C);
        RedJobs jb;
        jb.add(partials, 2, nb, s.sums);
        SBTV_TRY(s.book_start(jb, 1, C));                                // :29
    }
    SBTV_TRY(s.run.start());
    double t_enq = 1.0, c_enq = 0.0;                                     // t and the momentum factor as the next enqueue sees them
    auto enqueue = [&](int k) -> int {                                   // :34
        const int o = k & 1, p = o ^ 1;
        const double cm = c_enq;
        hipLaunchKernelGGL(fl1_momentum_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)zb[p],
                           (const double *)zb[o], cm, zy, P);
        SBTV_TRY(op_gradf(ctx, s.c, zy, s.acc, gi));                     // :38; its residual sum (of the momentum point) is not used
        SBTV_TRY(wav_analysis(ctx, wp, gi, g, 1));
        if (td)
            hipLaunchKernelGGL(fl1_step_kernel<true>, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)xb[p], xb[o],
                               (const double *)g, td, cm, invL, T, partials, C);
        else
            hipLaunchKernelGGL(fl1_step_kernel<false>, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)xb[p], xb[o],
                               (const double *)g, td, cm, invL, T, partials, C);
        SBTV_TRY(wav_synthesis(ctx, wp, xb[o], zb[o], 1));               // :43
        SBTV_TRY(op_resid(ctx, s.c, zb[o], s.acc));                      // :44
        const double t_old = t_enq;
        t_enq = 0.5 * (1 + sqrt(1 + 4 * t_old * t_old));                 // :41
        c_enq = (t_old - 1) / t_enq;                                     // :42
        RedJobs jb;
        jb.add(partials, nq, nb, s.sums);
        return s.reduce_and_publish(k, jb);
    };
    bool stop = false;
    // host side of iteration k: traces and the stop rule (:44-66)
    auto process = [&](int k) -> int {
        const double *hsl;
        SBTV_TRY(s.run.wait(k, &hsl));
        ctx->calls += 3;                                                 // A(y), AT, A(x)
        const double f = s.book(k - 1, hsl, 3, C);                       // :44-45
        double crit;
        if (stopcriterion == 1)
            crit = fabs(f - s.obj_prev) / f;                             // :51
        else if (stopcriterion == 2)
            crit = sqrt(hsl[2]) / sqrt(hsl[1]);                          // :53 (0 / 0 = NaN at x = 0: never below the tolerance)
        else
            crit = f;                                                    // :55
        s.obj_prev = f;
        stop = crit < tolerance;                                         // :64
        return 0;
    };
    int last = 1;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiters, lag, false, enqueue, process, [&] { return !stop; }));
    SBTV_TRY(s.run.finish(P, last, nullptr, nullptr));
    SBTV_HIP(ctx, hipMemcpyAsync(xw_out_dev, xb[last & 1], sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
    if (x_out_dev)
        SBTV_HIP(ctx, hipMemcpyAsync(x_out_dev, zb[last & 1], sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// image b of a batch as its solver sees it (device pointers; xw, x: null where the entry point has no such output)
struct WavItem {
    const double *y, *tru, *init;
    double *xw, *x;
};

// What the three entry points do once their arguments are checked and the frame is planned, in the spirit of admm_batch
// (these solvers have no sharded form and no exact repeat).  The unknown is the coefficient array (xw_out given: `tru`,
// `init` and xw_out have C = bands M N elements per image, x_out is optional) or the image (xw_out null: they have M N).
// The arrays are staged and the images solved one after another by one(b, item).
template <class One>
int wav_batch(sbtv_ctx *ctx, int M, int N, int batch, const WavPlan &wp, const double *y, const double *tru, const double *init,
              double *xw_out, double *x_out, int flags, One &&one) {
    SBTV_TRY(check_even_pixels(ctx, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    const size_t P = (size_t)M * N, C = P * wp.bands(), U = xw_out ? C : P;
    const double *yd = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", y, P * batch, flags, &yd));
    SBTV_TRY(stage_in(ctx, xw_out ? "wav.in.true" : "admm.in.true", tru, U * batch, flags, &td));
    SBTV_TRY(stage_in(ctx, xw_out ? "wav.in.xinit" : "admm.in.xinit", init, U * batch, flags, &xi));
    double *xwo = nullptr, *xo = nullptr;
    if (xw_out) SBTV_TRY(stage_out_buf(ctx, "wav.out.xw", xw_out, C * batch, flags, &xwo));
    if (x_out) SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, P * batch, flags, &xo));
    for (size_t b = 0; b < (size_t)batch; ++b)
        SBTV_TRY(one(b, WavItem{yd + b * P, off(td, b * U), off(xi, b * U), off(xwo, b * C), off(xo, b * P)}));
    if (xw_out) SBTV_TRY(stage_out_copy(ctx, xw_out, xwo, C * batch, flags));
    if (x_out) SBTV_TRY(stage_out_copy(ctx, x_out, xo, P * batch, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_SALSA_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                       const double *h, int hlen, int levels, const double *tau, const double *mu,
                       const sbtv_salsa_opts *opts, const double *true_xw, const double *xw_init, double *xw_out,
                       double *x_out, double *objective, double *distance, double *times, double *mses, int *numA,
                       int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "SALSA_wavelet", y, taps, opts, xw_init, M, N, batch, taille, "xw_init", false));   // no TV prox
    if (!tau || !mu || !xw_out) return fail(ctx, SBTV_ERR_BADARG, "SALSA_wavelet: missing required argument");
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    for (int b = 0; b < batch; ++b)
        if (!(mu[b] > 0.0)) return fail(ctx, SBTV_ERR_BADARG, "SALSA_wavelet: mu must be > 0");
    const size_t mi = (size_t)opts->maxiter;
    return wav_batch(ctx, M, N, batch, wp, y, true_xw, xw_init, xw_out, x_out, flags, [&](size_t b, const WavItem &it) {
        return wavelet_one(ctx, it.y, M, N, taps + b * taille * taille, taille, wp, tau[b], mu[b], opts, it.tru, it.init, it.xw,
                           it.x, off(objective, b * (mi + 1)), off(distance, b * mi), off(times, b * (mi + 1)),
                           off(mses, b * (mi + 1)), off(numA, b), off(numAt, b), off(n_outer, b));
    });
}

int sbtv_SALSA_analysis(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                        const double *h, int hlen, int levels, const double *tau, const double *mu,
                        const sbtv_salsa_opts *opts, const double *true_x, const double *x_init, double *x_out,
                        double *objective, double *distance, double *times, double *mses, int *numA, int *numAt,
                        int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "SALSA_analysis", y, taps, opts, x_init, M, N, batch, taille, "x_init", false));   // no TV prox
    if (!tau || !mu || !x_out) return fail(ctx, SBTV_ERR_BADARG, "SALSA_analysis: missing required argument");
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    for (int b = 0; b < batch; ++b)
        if (!(mu[b] > 0.0)) return fail(ctx, SBTV_ERR_BADARG, "SALSA_analysis: mu must be > 0");
    const size_t mi = (size_t)opts->maxiter;
    return wav_batch(ctx, M, N, batch, wp, y, true_x, x_init, nullptr, x_out, flags, [&](size_t b, const WavItem &it) {
        return analysis_one(ctx, it.y, M, N, taps + b * taille * taille, taille, wp, tau[b], mu[b], opts, it.tru, it.init, it.x,
                            off(objective, b * (mi + 1)), off(distance, b * mi), off(times, b * (mi + 1)),
                            off(mses, b * (mi + 1)), off(numA, b), off(numAt, b), off(n_outer, b));
    });
}

int sbtv_fista_l1(sbtv_ctx *ctx, const double *b, int M, int N, int batch, const double *taps, int taille, const double *h,
                  int hlen, int levels, const double *tau, double L, int stopcriterion, double tolerance, int maxiters,
                  const double *true_xw, const double *xw_init, double *xw_out, double *x_out, double *objective,
                  double *times, double *mses, int *n_iter, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!b || !taps || !h || !tau || !xw_out || batch < 1)
        return fail(ctx, SBTV_ERR_BADARG, "fista_l1: missing required argument (b, taps, h, tau, xw_out; batch >= 1)");
    if (stopcriterion < 1 || stopcriterion > 3) return fail(ctx, SBTV_ERR_STOPCRITERION, "Invalid stopping criterion!");   // :57
    if (maxiters < 1) return fail(ctx, SBTV_ERR_MAXITER, "fista_l1: maxiters must be positive");
    if (!std::isfinite(L) || !(L > 0.0)) return fail(ctx, SBTV_ERR_BADARG, "fista_l1: L must be finite and > 0");
    if (std::isnan(tolerance)) return fail(ctx, SBTV_ERR_BADARG, "fista_l1: tolerance is NaN");
    for (int i = 0; i < batch; ++i)
        if (!std::isfinite(tau[i]) || !(tau[i] >= 0.0)) return fail(ctx, SBTV_ERR_BADARG, "fista_l1: tau must be finite and >= 0");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    const size_t mi = (size_t)maxiters;
    const int lag = (flags & SBTV_FISTA_L1_NOLAG) ? 0 : 1;
    return wav_batch(ctx, M, N, batch, wp, b, true_xw, xw_init, xw_out, x_out, flags, [&](size_t i, const WavItem &it) {
        return fista_l1_one(ctx, it.y, M, N, taps + i * taille * taille, taille, wp, tau[i], L, stopcriterion, tolerance, maxiters,
                            lag, it.tru, it.init, it.xw, it.x, off(objective, i * mi), off(times, i * mi), off(mses, i * mi),
                            off(n_iter, i));
    });
}

}  // extern "C"

// Masked-observation SALSA with the wavelet analysis prior (sbtv_SALSA_masked_analysis):
//     min over the image x   0.5 sum(m .* (B x - y).^2) + tau ||W' x||_1
// B the circular blur of the taps, m non-negative weights (0 = not observed), W the Parseval frame of wavelet.hip.  It is the
// mask-decoupling ADMM of Almeida & Figueiredo (IEEE TIP 2013), which masked_one (admm.hip) runs with the TV regulariser, with
// the frame-analysis prior of analysis_one (wavelet_deconv.hip) in its place: the splits are u = W'x on the coefficients and
// v = Bx on the pixels, the multipliers follow SALSA_v2's sign convention (include/sbtv.h states the iteration).  Nothing here
// calls the TV prox.  The frame transforms, the coefficient pass (wav_astep_kernel, wav_step.inc), the two-input spectral solve
// and the second row pass that yields Bx are those of the two parents; what is new is one pixel pass (ma_pixel_kernel) and the
// loop that joins them on one stream (AdmmRun, admm_run.inc).  DESIGN.md §3.21.
#include <chrono>
#include <cmath>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

#include "admm_run.inc"    // AB, ad_store_partials, AD_LOOP / AD_LD / AD_ST, ad_blocks, admm_common, upload_par, AdmmRun
#include "wav_step.inc"    // wav_astep_kernel
#include "masked_my.inc"   // masked_my_kernel

// The one pixel pass of an outer iteration k, after the two inverse transforms (x_k, Bx_k), on the v_k this iteration solved
// with and bv_{k-1}:
//   bv' = bv + (v - Bx) ; v' = (m .* y + mu2 (Bx - bv')) ./ (m + mu2), the v of iteration k + 1
//   partials [7][nb]: m (Bx-y)^2, (Bx-v)^2, Bx^2, v^2, x^2, (x-true)^2, (x-xprev)^2
// x, tru and xprev may each be null: a null array is neither read nor summed (x without tru and xprev: x^2 alone).  The start
// is the same pass with v = Bx_0 and bv = 0.  Five arrays read, two written: 56 B per pixel.
__global__ __launch_bounds__(AB) void ma_pixel_kernel(const double *__restrict__ Bx, const double *__restrict__ y,
                                                       const double *__restrict__ m, double *__restrict__ v,
                                                       double *__restrict__ bv, const double *__restrict__ x,
                                                       const double *__restrict__ tru, const double *__restrict__ xprev,
                                                       double mu2, double *__restrict__ partials, size_t P) {
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    AD_LOOP(q, P) {
        const double2 ax = AD_LD(Bx, q), vv = AD_LD(v, q), yv = AD_LD(y, q), mv = AD_LD(m, q);
        double2 b2 = AD_LD(bv, q);
        b2.x = b2.x + (vv.x - ax.x);
        b2.y = b2.y + (vv.y - ax.y);
        AD_ST(bv, q, b2);
        AD_ST(v, q, make_double2((mv.x * yv.x + mu2 * (ax.x - b2.x)) / (mv.x + mu2),
                                 (mv.y * yv.y + mu2 * (ax.y - b2.y)) / (mv.y + mu2)));
        {
            const double e0 = ax.x - yv.x, e1 = ax.y - yv.y;
            acc[0] += mv.x * (e0 * e0) + mv.y * (e1 * e1);
            const double r0 = ax.x - vv.x, r1 = ax.y - vv.y;
            acc[1] += r0 * r0 + r1 * r1;
        }
        acc[2] += ax.x * ax.x + ax.y * ax.y;
        acc[3] += vv.x * vv.x + vv.y * vv.y;
        if (x) {
            const double2 xv = AD_LD(x, q);
            acc[4] += xv.x * xv.x + xv.y * xv.y;
            if (tru) {
                const double2 tv = AD_LD(tru, q);
                const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
                acc[5] += m0 * m0 + m1 * m1;
            }
            if (xprev) {
                const double2 xo = AD_LD(xprev, q);
                const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
                acc[6] += m0 * m0 + m1 * m1;
            }
        }
    }
    ad_store_partials<7>(acc, partials);
}

// ------------------------------------------------------------------------------------------------
// One image.  The iteration of include/sbtv.h on the coefficient state (s, bu), s = u + bu, as analysis_one keeps it (u is
// never stored), and the pixel state x, Bx, v, bv as masked_one keeps it.  One outer iteration k on one stream:
//     z  = W s_k                                                    wav_synthesis
//     Ws = fft2(v_k + bv_{k-1})                                     op_spectrum
//     X  = (conj(H) Ws + r fft2(z)) / (|H|^2 + r), r = mu1 / mu2    op_solve (the row pass OP_SALSA with Ws in the place of
//     x_k = real(ifft2(X))                                          fft2(y) and r in the place of mu, as in masked_one)
//     Bx_k = real(ifft2(H X))                                       a second row pass OP_MUL_H on the spectrum the first left,
//                                                                   one inverse column pass: no forward transform
//     w  = W' x_k                                                   wav_analysis
//     u_k = s_k - bu_{k-1}, its sums, bu_k, s_{k+1}                 wav_astep_kernel, T = tau / mu1
//     bv_k, v_{k+1}, the sums of the pixels                         ma_pixel_kernel
//     one reduction launch, publish
// s, bu and x are double-buffered, so the result of the stopping iteration is intact when the host evaluates the stop rule one
// iteration late (opts->speculate bit 0); Bx, v and bv have one buffer each: the iteration after the stopping one overwrites
// them, and nobody reads them again.  x is read by the pixel pass only with TRUE_X or stop rule 2, xprev only under rule 2.
// partials: [0..3] step sums, nb each, then [0..6] pixel sums, nbp each
// sums: [0] |u|, [1] u^2, [2] (w-u)^2, [3] w^2, [4] m (Bx-y)^2, [5] (Bx-v)^2, [6] Bx^2, [7] v^2, [8] x^2, [9] (x-true)^2,
//       [10] (x-xprev)^2
int masked_analysis_one(sbtv_ctx *ctx, const double *yd, const double *md, int M, int N, const double *taps, int taille,
                        const WavPlan &wp, double tau, double mu1, double mu2, const sbtv_salsa_opts *opts, const double *td,
                        const double *xi, double *x_out_dev, double *objective, double *distance, double *times, double *mses,
                        int *numA, int *numAt, int *n_outer) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, nullptr, &c));
    const size_t P = c.P, C = P * wp.bands();
    const int nb = ad_blocks(C), nbp = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    double *sbuf[2], *bbuf[2], *xbuf[2], *w, *z, *v, *bv, *Bx, *par, *partials, *sums, *acc;
    double2 *Ws, *S2;
    SBTV_TRY(ws_get_t(ctx, "wav.s0", C, &sbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.s1", C, &sbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "wav.we0", C, &bbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.we1", C, &bbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "wav.w", C, &w));
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &z));
    SBTV_TRY(ws_get_t(ctx, "admm.v", P, &v));
    SBTV_TRY(ws_get_t(ctx, "admm.bv", P, &bv));
    SBTV_TRY(ws_get_t(ctx, "admm.Ax", P, &Bx));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu1 / mu2
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * 1024, &partials));
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));         // residual sum of OP_SALSA (against Ws: not used)
    SBTV_TRY(ws_get_t(ctx, "admm.W", c.fp.u_img, &Ws));
    SBTV_TRY(ws_get_t(ctx, "admm.S2", c.fp.s_img, &S2));
    double *const ppix = partials + (size_t)4 * nb;
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    SBTV_TRY(upload_par(ctx, par, {mu1 / mu2, 0.0, 0.0, 0.0}));
    const double T = tau / mu1;
    const bool rule2 = opts->stopcriterion == 2;
    // the inverse column pass of H X takes the spectrum the row pass of X left: N times the column transform of x (the
    // chirp-z path keeps whole 2-D spectra, its "row pass" is point-wise)
    const double bx_scale = c.fp.generic ? c.inv_scale : c.inv_scale / (double)N;
    // the two passes and the jobs of their partials; x is handed to the pixel pass only where one of its sums is wanted
    auto passes = [&](const double *sp, const double *bp, double *bn, double *sn, const double *xn, const double *xprev,
                      RedJobs &jb) {
        hipLaunchKernelGGL(wav_astep_kernel, dim3(nb), dim3(AB), 0, ctx->stream, sp, bp, (const double *)w, bn, sn, T, partials,
                           C);
        const bool wantx = td || xprev;
        hipLaunchKernelGGL(ma_pixel_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)Bx, yd, md, v, bv,
                           wantx ? xn : (const double *)nullptr, td, xprev, mu2, ppix, P);
        jb.add(partials, 4, nb, sums);
        jb.add(ppix, 7, nbp, sums + 4);
    };
    double *x = xbuf[0];
    if (opts->initialization == 2) {                                     // x = B'(m .* y)
        hipLaunchKernelGGL(masked_my_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, md, yd, z, P);
        SBTV_TRY(op_apply(ctx, c, OP_MUL_HC, z, x));
        run.numAt += 1;
        ctx->calls += 1;
    } else {
        SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, x));
    }
    // Bx = B x ; PTx = W'x ; u = PTx ; bu = 0 ; v = Bx ; bv = 0.  The two passes on (s, bu) = (w_0, 0) and (v, bv) = (Bx_0, 0)
    // leave bu = bv = 0, the first s, the first v and the sums of objective(1) / mses(1)
    SBTV_TRY(op_apply(ctx, c, OP_MUL_H, x, Bx));
    run.numA += 1;
    ctx->calls += 1;
    double obj_prev;
    {
        SBTV_TRY(wav_analysis(ctx, wp, x, w, 1));
        SBTV_HIP(ctx, hipMemsetAsync(bbuf[1], 0, sizeof(double) * C, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(v, Bx, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(bv, 0, sizeof(double) * P, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));
        RedJobs jb;
        passes(w, bbuf[1], bbuf[0], sbuf[0], x, nullptr, jb);
        SBTV_TRY(reduce_jobs(ctx, jb));
        SBTV_HIP(ctx, hipGetLastError());
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        obj_prev = 0.5 * hs[4] + tau * hs[0];
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[9] / (double)P;
    }
    SBTV_TRY(run.start());
    const int lag = (opts->speculate & 1) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {
        const int o = outer & 1, p = o ^ 1;
        double *xn = xbuf[o];
        SBTV_TRY(wav_synthesis(ctx, wp, sbuf[p], z, 1));                 // W(u + bu)
        SBTV_TRY(op_spectrum(ctx, c.fp, v, bv, S2, Ws));                 // fft2(v + bv): v from the previous pixel pass
        SBTV_TRY(op_solve(ctx, c, z, nullptr, Ws, par, acc, xn));        // r = mu1 / mu2
        // Bx = real(ifft2(H X)) from the column-transformed x the row pass left in S
        {
            RowsArgs a{};
            a.dir_fwd = 1;
            a.dir_inv = 1;
            a.op = OP_MUL_H;
            a.H = c.Hs;
            SBTV_TRY(fft_rows(ctx, c.fp, c.S, S2, a));
            SBTV_TRY(fft_cols_inv(ctx, c.fp, S2, Bx, bx_scale));
        }
        SBTV_TRY(wav_analysis(ctx, wp, xn, w, 1));
        RedJobs jb;
        passes(sbuf[p], bbuf[p], bbuf[o], sbuf[o], xn, rule2 ? (const double *)xbuf[p] : (const double *)nullptr, jb);
        SBTV_TRY(reduce_jobs(ctx, jb));
        return run.publish(outer, sums, 12, 0);
    };
    bool stop = false;
    // host side of iteration `outer`: traces and the stop rule of SALSA_v2.m:442-482
    auto process = [&](int outer) -> int {
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        run.numA += 1;                                                   // H .* X
        run.numAt += 1;                                                  // conj(H) .* fft2(v + bv)
        ctx->calls += 2;
        const double f = 0.5 * hsl[4] + tau * hsl[0];
        if (objective) objective[outer] = f;
        if (mses && td) mses[outer] = hsl[9] / (double)P;
        if (distance) {
            distance[(size_t)(outer - 1) * 2] = sqrt(hsl[2]) / sqrt(hsl[3] + hsl[1]);
            distance[(size_t)(outer - 1) * 2 + 1] = sqrt(hsl[5]) / sqrt(hsl[6] + hsl[7]);
        }
        if (times) times[outer] = run.seconds();
        stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[10], hsl[8], opts->tolA);
        obj_prev = f;
        return 0;
    };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, opts->maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[last & 1], x_out_dev);
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_SALSA_masked_analysis(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch, const double *taps,
                               int taille, const double *h, int hlen, int levels, const double *tau, const double *mu1,
                               const double *mu2, const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                               double *x_out, double *objective, double *distance, double *times, double *mses, int *numA,
                               int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "SALSA_masked_analysis", y, taps, opts, x_init, M, N, batch, taille, "x_init", false));   // no TV prox
    if (!mask) return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked_analysis: the mask is missing");
    if (!tau || !mu1 || !mu2 || !x_out) return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked_analysis: missing required argument");
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0))
            return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked_analysis: mu1, mu2 must be > 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    const size_t P = (size_t)M * N, cnt = P * batch, t2 = (size_t)taille * taille, mi = (size_t)opts->maxiter;
    if (!(flags & SBTV_DEVICE_PTRS))
        for (size_t i = 0; i < cnt; ++i)
            if (!(mask[i] >= 0.0) || std::isinf(mask[i]))
                return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked_analysis: the mask must be finite and non-negative");
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    // no sharded form: the arrays are staged and the images solved one after another
    const double *yd = nullptr, *md = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "admm.in.mask", mask, cnt, flags, &md));
    SBTV_TRY(stage_in(ctx, "admm.in.true", true_x, cnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "admm.in.xinit", x_init, cnt, flags, &xi));
    double *xo = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, cnt, flags, &xo));
    for (size_t b = 0; b < (size_t)batch; ++b) {
        const size_t o = b * P;
        SBTV_TRY(masked_analysis_one(ctx, yd + o, md + o, M, N, taps + b * t2, taille, wp, tau[b], mu1[b], mu2[b], opts,
                                     off(td, o), off(xi, o), xo + o, off(objective, b * (mi + 1)), off(distance, b * mi * 2),
                                     off(times, b * (mi + 1)), off(mses, b * (mi + 1)), off(numA, b), off(numAt, b),
                                     off(n_outer, b)));
    }
    SBTV_TRY(stage_out_copy(ctx, x_out, xo, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

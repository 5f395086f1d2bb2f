// CoRAL with the compound regulariser it exists for (SALSA/CoRAL_v2.m:2-476): TV on the image plus l1 on the coefficients of
// the Parseval frame W of wavelet.hip,
//     min over x   0.5 ||y - B x||^2 + tau1 TV(x) + tau2 ||W' x||_1                                  (sbtv_CoRAL_wavelet)
// i.e. P1 = P1' = identity with TVINITIALIZATION1 = 1, P2 = W = mirdwt_TI2D, P2' = W' = mrdwt_TI2D, Psi2 = soft, Phi2 = l1 and
// invLS(r) = real(ifft2(fft2(r) ./ (|H|^2 + mu1 + mu2))), the exact x-minimiser because W W' = I.  It joins the two halves of
// the library: the warm-started Chambolle prox with optimistic launches of the ADMM front-ends (AdmmProx, admm_prox.inc) and
// the coefficient state and step pass of the analysis-prior wavelet SALSA (wav_astep_kernel, wav_step.inc), in one pipelined
// loop on one stream (AdmmRun, admm_run.inc).  DESIGN.md §3.19.
#include <chrono>
#include <cmath>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

#include "admm_run.inc"   // AB, ad_store_partials, AD_LOOP / AD_LD / AD_ST, ad_sub_kernel, ad_blocks, admm_common, upload_par, AdmmRun
#include "admm_prox.inc"  // AdmmProx
#include "wav_step.inc"   // wav_init_kernel, wav_astep_kernel

// s = (mu1 (u + bu) + mu2 z) / mu_ls, z = W(v + bv)                          (CoRAL_v2.m:411, ATy enters spectrally)
// TVS: also the periodic TV norm of u (utils/TVnorm.m:2) for the objective (:425), partials [1][nb]: u is in flight here
// anyway (M even; element 2q = (i, j) with i even)
template <bool TVS>
__global__ __launch_bounds__(AB) void cw_s_kernel(const double *__restrict__ u, const double *__restrict__ bu,
                                                   const double *__restrict__ z, double mu1, double mu2, double mu_ls,
                                                   double *__restrict__ s, double *__restrict__ partials, unsigned M,
                                                   unsigned N, size_t P) {
    double acc[1] = {0.0};
    AD_LOOP(q, P) {
        const double2 a = AD_LD(u, q), b = AD_LD(bu, q), c = AD_LD(z, q);
        AD_ST(s, q, make_double2((mu1 * (a.x + b.x) + mu2 * c.x) / mu_ls, (mu1 * (a.y + b.y) + mu2 * c.y) / mu_ls));
        if constexpr (TVS) {
            const unsigned idx = (unsigned)(2 * q), j = idx / M, i = idx - j * M;
            const size_t lcol = (size_t)(j > 0 ? j - 1 : N - 1) * M + i, up = (size_t)j * M + (i > 0 ? i - 1 : M - 1);
            const double2 ul = *reinterpret_cast<const double2 *>(u + lcol);
            const double uu = u[up];
            const double h0 = a.x - ul.x, v0 = a.x - uu, h1 = a.y - ul.y, v1 = a.y - a.x;
            acc[0] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
        }
    }
    if constexpr (TVS) ad_store_partials<1>(acc, partials);
}

// bu += u - x ; g1 = x - bu  (:420 and the next prox input :401)
//   partials [5][nb]: (x-true)^2, (x-u)^2, x^2, u^2, (x-xprev)^2 (tru / xprev null: not read, not summed)
__global__ __launch_bounds__(AB) void cw_post_kernel(const double *__restrict__ x, const double *__restrict__ xprev,
                                                      const double *__restrict__ u, double *__restrict__ bu,
                                                      double *__restrict__ g1, const double *__restrict__ tru,
                                                      double *__restrict__ partials, size_t P) {
    double acc[5] = {0, 0, 0, 0, 0};
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), uv = AD_LD(u, q);
        double2 b1 = AD_LD(bu, q);
        b1.x = b1.x + (uv.x - xv.x);
        b1.y = b1.y + (uv.y - xv.y);
        AD_ST(bu, q, b1);
        AD_ST(g1, q, make_double2(xv.x - b1.x, xv.y - b1.y));
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[0] += m0 * m0 + m1 * m1;
        }
        {
            const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
            acc[1] += d0 * d0 + d1 * d1;
        }
        acc[2] += xv.x * xv.x + xv.y * xv.y;
        acc[3] += uv.x * uv.x + uv.y * uv.y;
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[4] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<5>(acc, partials);
}

// ------------------------------------------------------------------------------------------------
// One image.  The reference's iteration (CoRAL_v2.m:349-476) with the splits u = x (TV) and v = W'x (l1):
//     start:  u = x ; bu = u ; v = W'x ; bv = v ; zero duals                                                   (:349-361,384-392)
//     outer:  u = chambolle_prox_TV_stop(x - bu, tau1/mu1) ; v = soft(W'x - bv, tau2/mu2)                      (:401,408)
//             x = invLS(B'y + mu1 (u + bu) + mu2 W(v + bv)) ; bu += u - x ; bv += v - W'x                      (:411-421)
// What runs keeps the pixel state x (double-buffered), u, bu, g1 = x - bu and the coefficient state (sv, bv), sv = v + bv
// (double-buffered), as analysis_one does.  The start is sv_1 = bv_0 = W'x_0: the first soft argument W'x_0 - bv_0 is exactly
// zero, as the first prox input x_0 - bu_0 is.  One outer iteration k:
//     u = prox(g1)                                                   AdmmProx: optimistic from outer 2 on, else exact
//     z = W sv_k                                                     wav_synthesis
//     s = (mu1 (u + bu) + mu2 z) / mu, TV(u) riding along            cw_s_kernel
//     X = (conj(H) fft2(y) + mu fft2(s)) / (|H|^2 + mu) ; x_k        op_solve, ||y - B x_k||^2 by Parseval
//     w = W'x_k                                                      wav_analysis
//     v_k = sv_k - bv_{k-1}, its sums, bv_k, sv_{k+1}                wav_astep_kernel with T = tau2/mu2
//     bu += u - x_k ; g1 = x_k - bu ; the pixel sums                 cw_post_kernel
//     one reduction launch, publish
// The host books the traces one iteration late (opts->speculate bit 0).
// pix: [0..4] post sums, [5] TV(u), nbp each; cof: [0..3] step sums, nb each
// sums: [0..4] post sums, [5] TV(u), [8] resid2, [10..13] |v|, v^2, (w-v)^2, w^2, [16..] the step sums of an optimistic prox
int coral_wavelet_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, const WavPlan &wp,
                      double tau1, double tau2, double mu1, double mu2, const sbtv_salsa_opts *opts, const double *td,
                      const double *xi, double *x_out_dev, double *objective, double *distance, double *times, double *mses,
                      int *numA, int *numAt, int *n_outer, bool spec_wanted) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, yd, &c));
    const int K = opts->TViters;
    AdmmProx prox;
    SBTV_TRY(prox.plan(ctx, M, N, 1, "prox", K, opts));
    const size_t P = c.P, C = P * wp.bands();
    const int nb = ad_blocks(C), nbp = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    const bool tv_in_s = !(M & 1) && P < ((size_t)1 << 31);             // TV(u) rides in the pass that forms s
    const double mu_ls = mu1 + mu2, T2 = tau2 / mu2;                     // :137, :361
    double *xbuf[2], *sbuf[2], *bbuf[2], *u, *bu, *z, *s, *g1, *w, *par, *pix, *cof, *sums, *acc;
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &u));
    SBTV_TRY(ws_get_t(ctx, "admm.bu", P, &bu));
    SBTV_TRY(ws_get_t(ctx, "admm.v", P, &z));
    SBTV_TRY(ws_get_t(ctx, "admm.w", P, &s));
    SBTV_TRY(ws_get_t(ctx, "admm.g", P, &g1));
    SBTV_TRY(ws_get_t(ctx, "wav.s0", C, &sbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.s1", C, &sbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "wav.we0", C, &bbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.we1", C, &bbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "wav.w", C, &w));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu_ls, thr1
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * 1024, &pix));
    cof = pix + (size_t)6 * nbp;
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    SBTV_TRY(upload_par(ctx, par, {mu_ls, tau1 / mu1, 0.0, 0.0}));      // threshold :356
    prox.lam = par + 1;
    const int maxiter = opts->maxiter;
    const bool rule2 = opts->stopcriterion == 2;
    run.numAt = 2;                                                       // ATy twice (:189,219)
    ctx->calls += 3;                                                     // AT(y), invLS(ATy), AT(y)
    double *x = xbuf[0];
    SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, x));
    if (opts->initialization == 0) ctx->calls += 1;
    // u = x ; bu = u (:353-356) -> first prox input x - bu = 0 ; v = W'x ; bv = v (:358-361) -> sv_1 = 0 + bv_0 = W'x
    for (double *dst : {u, bu}) SBTV_HIP(ctx, hipMemcpyAsync(dst, x, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(g1, 0, sizeof(double) * P, ctx->stream));
    SBTV_TRY(wav_analysis(ctx, wp, x, sbuf[0], 1));
    SBTV_HIP(ctx, hipMemcpyAsync(bbuf[0], sbuf[0], sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(prox_zero_duals(ctx, prox.pp));                             // :384-392
    SBTV_TRY(prox.arm(ctx, true));

    // initial objective (:366-368) and mses(1) (:381)
    double obj_prev;
    {
        SBTV_TRY(op_resid(ctx, c, x, acc));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));
        hipLaunchKernelGGL(wav_init_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)sbuf[0], (const double *)nullptr,
                           cof, C);
        RedJobs jb;
        jb.add(cof, 1, nb, sums + 10);
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 5));
        if (td) {
            double *o4 = nullptr;
            SBTV_TRY(ws_get_t(ctx, "admm.o4", (size_t)4, &o4));
            SBTV_TRY(pair_sums(ctx, x, td, P, 1, o4));
            SBTV_HIP(ctx, hipMemcpyAsync(sums, o4, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        }
        SBTV_HIP(ctx, hipGetLastError());
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        run.numA += 1;
        ctx->calls += 1;
        obj_prev = 0.5 * (hs[8] * c.parseval) + tau1 * hs[5] + tau2 * hs[10];
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[0] / (double)P;
    }
    SBTV_TRY(run.start());
    const bool spec = spec_wanted && prox_spec_ok(prox.pp, g1, u, K);
    const int lag = (spec && (opts->speculate & 1)) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {                               // :394
        const int o = outer & 1, p = o ^ 1;
        double *xn = xbuf[o];
        const double *xprev = xbuf[p];
        // the TV prox with its warm-started duals (:401).  The first outer iteration always runs exactly: its input x - bu is
        // zero and the rule stops at k = 1; the control block is re-armed afterwards
        const bool sp = spec && outer >= 2;
        RedJobs jb;
        if (spec && outer == 2) SBTV_TRY(prox.arm(ctx, false));
        SBTV_TRY(prox.run(ctx, g1, u, sp, sums + 16, &jb));
        // r = ATy + mu1 (u+bu) + mu2 W(v+bv) ; x = invLS(r)   (:411-413)  + residual energy (:423, Parseval)
        SBTV_TRY(wav_synthesis(ctx, wp, sbuf[p], z, 1));
        if (tv_in_s)
            hipLaunchKernelGGL(cw_s_kernel<true>, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)u, (const double *)bu,
                               (const double *)z, mu1, mu2, mu_ls, s, pix + (size_t)5 * nbp, (unsigned)M, (unsigned)N, P);
        else
            hipLaunchKernelGGL(cw_s_kernel<false>, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)u, (const double *)bu,
                               (const double *)z, mu1, mu2, mu_ls, s, pix + (size_t)5 * nbp, (unsigned)M, (unsigned)N, P);
        SBTV_TRY(op_solve(ctx, c, s, nullptr, c.Ys, par, acc, xn));    // mu_ls
        // W'x ; v = sv - bv, its sums ; bv += v - W'x ; the next sv = soft(W'x - bv, tau2/mu2) + bv   (:408 of outer + 1, :421)
        SBTV_TRY(wav_analysis(ctx, wp, xn, w, 1));
        hipLaunchKernelGGL(wav_astep_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)sbuf[p], (const double *)bbuf[p],
                           (const double *)w, bbuf[o], sbuf[o], T2, cof, C);
        hipLaunchKernelGGL(cw_post_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)xn,
                           rule2 ? xprev : (const double *)nullptr, (const double *)u, bu, g1, td, pix, P);
        jb.add(pix, tv_in_s ? 6 : 5, nbp, sums);
        jb.add(cof, 4, nb, sums + 10);
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        if (!tv_in_s) SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 5));
        if (sp) return run.publish(outer, sums, 16 + K, K);
        return run.publish(outer, sums, 16, 0, prox.pp.ctrl);
    };
    bool stop = false;
    auto process = [&](int outer) -> int {
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        if (spec && outer >= 2) SBTV_TRY(prox.check(ctx, hsl + 16));
        run.numA += 1;
        ctx->calls += 2;                                                 // invLS, A
        const double f = 0.5 * (hsl[8] * c.parseval) + tau1 * hsl[5] + tau2 * hsl[10];       // :425
        if (objective) objective[outer] = f;
        if (mses && td) mses[outer] = hsl[0] / (double)P;                // :428-429
        if (distance) {
            distance[(size_t)(outer - 1) * 2] = sqrt(hsl[1]) / sqrt(hsl[2] + hsl[3]);        // :432
            distance[(size_t)(outer - 1) * 2 + 1] = sqrt(hsl[12]) / sqrt(hsl[13] + hsl[11]);  // :433
        }
        if (times) times[outer] = run.seconds();
        stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[4], hsl[2], opts->tolA);
        obj_prev = f;
        return 0;
    };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[last & 1], x_out_dev);
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_CoRAL_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                       const double *h, int hlen, int levels, const double *tau1, const double *tau2, const double *mu1,
                       const double *mu2, const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                       double *x_out, double *objective, double *distance, double *times, double *mses, int *numA,
                       int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "CoRAL_wavelet", y, taps, opts, x_init, M, N, batch, taille));
    if (!tau1 || !tau2 || !mu1 || !mu2 || !x_out) return fail(ctx, SBTV_ERR_BADARG, "CoRAL_wavelet: missing required argument");
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0))
            return fail(ctx, SBTV_ERR_MISSING_LS, "(A^T A + mu I)^(-1) must be specified: mu1, mu2 must be > 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    // no sharded form: the arrays are staged and the images solved one after another, optimistic prox launches first (unless
    // bit 1 of `speculate` asks for exact ones), exact ones if the rule fired early
    const size_t P = (size_t)M * N, cnt = P * batch, t2 = (size_t)taille * taille, mi = (size_t)opts->maxiter;
    const double *yd = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "admm.in.true", true_x, cnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "admm.in.xinit", x_init, cnt, flags, &xi));
    double *xo = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, cnt, flags, &xo));
    for (size_t b = 0; b < (size_t)batch; ++b) {
        const size_t o = b * P;
        SBTV_TRY(solve_with_exact_repeat(ctx, !(opts->speculate & 2), [&](bool spec) {
            return coral_wavelet_one(ctx, yd + o, M, N, taps + b * t2, taille, wp, tau1[b], tau2[b], mu1[b], mu2[b], opts,
                                     off(td, o), off(xi, o), xo + o, off(objective, b * (mi + 1)), off(distance, b * mi * 2),
                                     off(times, b * (mi + 1)), off(mses, b * (mi + 1)), off(numA, b), off(numAt, b),
                                     off(n_outer, b), spec);
        }));
    }
    SBTV_TRY(stage_out_copy(ctx, x_out, xo, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

// C-SALSA with the wavelet analysis prior, the 'P' / 'PT' mode of SALSA/CSALSA_v2.m (:111-114, 208-213, 402, 467-478, 492):
//     min over the image x   ||W' x||_1    s.t.   ||B x - y||_2 <= epsilon                              (sbtv_CSALSA_wavelet)
// W the Parseval frame of wavelet.hip, i.e. TVINITIALIZATION = 0, Psi = soft with the threshold 1 / mu1 (:478), A = B, AT = B',
// PT = W' = mrdwt_TI2D, P = W = mirdwt_TI2D and invLS(r, mu1) = real(ifft2(fft2(r) ./ (|H|^2 + mu1))) as sbtv_CSALSA_v2 defines it:
// the exact x-minimiser for mu2 = 1 only; other mu2 run as the reference would run them.  The caller knows the noise level
// (epsilon = sqrt(n + 8 sqrt n) sigma by default, :413), not a regularisation parameter.  It joins the constraint split of
// csalsa_one (admm.hip; csalsa_step.inc) and the frame transforms and coefficient state of analysis_one (wavelet_deconv.hip) in
// one pipelined loop on one stream (AdmmRun, admm_run.inc).  DESIGN.md §3.20.
// One stated deviation: objective(k) = ||W' x_k||_1, the problem's objective, where the reference records phi(x) of the IMAGE
// (:423, 498).
#include <chrono>
#include <cmath>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

#include "admm_run.inc"     // AB, ad_store_partials, AD_LOOP / AD_LD / AD_ST, ad_blocks, admm_common, upload_par, AdmmRun
#include "csalsa_step.inc"  // csalsa_w_kernel, csalsa_ve_kernel, csalsa_scal_kernel, csalsa_spectral_wanted
#include "wav_step.inc"     // wav_init_kernel, wav_cstep_kernel
#include "ad_xsums.inc"     // ad_xsums_kernel

// The constraint split of the image form alone (:483-491, 494-495): ve = Ax - y - bv ; v = ve, or its projection on the epsilon
// ball ; bv <- bv - (Ax - y - v).  nve2: ||ve||^2 (device, from csalsa_ve_kernel).  partials [2][nb]: (Ax-y)^2, (Ax-y-v)^2
__global__ __launch_bounds__(AB) void csalsa_split_kernel(const double *__restrict__ Ax, const double *__restrict__ y,
                                                           double *__restrict__ v, double *__restrict__ bv,
                                                           const double *__restrict__ nve2, double eps,
                                                           double *__restrict__ partials, size_t P) {
    const double n_ve = sqrt(nve2[0]);
    const bool inside = n_ve <= eps;
    double acc[2] = {0.0, 0.0};
    AD_LOOP(q, P) {
        const double2 a = AD_LD(Ax, q), yy = AD_LD(y, q), c = AD_LD(bv, q);
        const double t0 = a.x - yy.x, t1 = a.y - yy.y;
        const double e0 = t0 - c.x, e1 = t1 - c.y;
        const double v0 = inside ? e0 : e0 / n_ve * eps, v1 = inside ? e1 : e1 / n_ve * eps;
        AD_ST(v, q, make_double2(v0, v1));
        const double r0 = t0 - v0, r1 = t1 - v1;
        AD_ST(bv, q, make_double2(c.x - r0, c.y - r1));
        acc[0] += t0 * t0 + t1 * t1;
        acc[1] += r0 * r0 + r1 * r1;
    }
    ad_store_partials<2>(acc, partials);
}

// ------------------------------------------------------------------------------------------------
// One image.  The reference's iteration (CSALSA_v2.m:401-561) with the splits u = W'x (l1) and v = Bx - y (the ball):
//     start:  u = bu = 0 (coefficients) ; v = bv = 0 (pixels)                                                     (:402-408)
//     outer:  x = invLS(mu1 W(u + bu) + mu2 B'(y + v + bv), mu1) ; u = soft(W'x - bu, 1/mu1)                      (:467-478)
//             ve = Bx - y - bv ; v = ve min(1, epsilon / ||ve||) ; bv -= Bx - y - v ; bu -= W'x - u               (:481-492)
// What runs keeps the image x (double-buffered: the host sees the stop rule one iteration late, opts->speculate bit 0) and
// the coefficient state (s, bu), s = u + bu.  Only x is returned, so s and bu have one buffer each: the iteration after the
// stopping one overwrites them, and nobody reads them again.  The constraint split is, by default, the spectrum E of ve and
// the scalar s_ = min(1, epsilon / ||ve||) of csalsa_one.  One outer iteration k of that spectral form:
//     z = W s                                                          wav_synthesis
//     S = fft2(z) ; the row pass OP_CSALSA ; x_k = real(ifft2(X))      fft_cols_fwd, fft_rows, fft_cols_inv
//     projection factor, next row-pass coefficients, two traces        csalsa_scal_kernel
//     w = W'x_k                                                        wav_analysis
//     u, bu, the next s, ||w||_1 and ||w - u||^2                       wav_cstep_kernel (wav_step.inc), T = 1/mu1
//     the sums over x_k, only with TRUE_X or stop rule 2               ad_xsums_kernel
//     one reduction launch, publish
// The image form keeps v and bv as images: a continuation factor != 1 (mu1, mu2 and the threshold change every iteration, and
// the host evaluates each iteration before it enqueues the next), plans without OP_CSALSA (the chirp-z sizes), or
// SBTV_CSALSA_SPECTRAL=0.  Per iteration: csalsa_w_kernel, op_spectrum, the synthesis, op_solve, the analysis, the same step
// pass, op_apply(OP_MUL_H), csalsa_ve_kernel with its reduction, csalsa_split_kernel.
// partials: [0..1] step sums, nb each, then [0..2] pixel sums, [0..1] split sums and ||ve||^2, nbp each
// sums: [0] ||Ax-y||^2, [1] ||Ax-y-v||^2, [2] ||w||_1, [3] ||w-u||^2, [4..6] (x-true)^2, (x-xprev)^2, x^2, [8] ||ve||^2
int csalsa_wavelet_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, const WavPlan &wp,
                       double mu1, double mu2, double sigma, double epsilon, double delta, const sbtv_salsa_opts *opts,
                       const double *td, const double *xi, double *x_out_dev, double *objective, double *distance1,
                       double *distance2, double *criterion, double *times, double *mses, int *numA, int *numAt, int *n_outer) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, yd, &c));
    // the spectral form needs fixed mu1 / mu2, an even M and the row kernels that carry OP_CSALSA, as in csalsa_one
    const bool spectral = delta == 1.0 && csalsa_spectral_wanted() && fft_rows_csalsa_ok(c.fp) && !(M & 1) &&
                          (size_t)M * N < ((size_t)1 << 31);
    const size_t P = c.P, C = P * wp.bands();
    const int nb = ad_blocks(C), nbp = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    double *xbuf[2], *s, *bu, *w, *z, *v = nullptr, *bv = nullptr, *wi = nullptr, *Ax = nullptr;
    double *par, *partials, *sums, *acc, *cst;
    double2 *Ws;
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &z));
    SBTV_TRY(ws_get_t(ctx, "wav.s0", C, &s));
    SBTV_TRY(ws_get_t(ctx, "wav.we0", C, &bu));
    SBTV_TRY(ws_get_t(ctx, "wav.w", C, &w));
    if (!spectral) {
        SBTV_TRY(ws_get_t(ctx, "admm.v", P, &v));
        SBTV_TRY(ws_get_t(ctx, "admm.bv", P, &bv));
        SBTV_TRY(ws_get_t(ctx, "admm.w", P, &wi));
        SBTV_TRY(ws_get_t(ctx, "admm.Ax", P, &Ax));
    }
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu1, mu2, 1/mu1
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * 1024, &partials));
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));
    SBTV_TRY(ws_get_t(ctx, "admm.W", c.fp.u_img, &Ws));                 // fft2(mu2 (y+v+bv)), or the state spectrum E
    SBTV_TRY(ws_get_t(ctx, "admm.cs", (size_t)8, &cst));
    double2 *const Es = Ws;
    double *const ppix = partials + (size_t)2 * nb, *const psplit = ppix + (size_t)3 * nbp, *const pve = psplit + (size_t)2 * nbp;
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    const int maxiter = opts->maxiter;
    const bool rule2 = opts->stopcriterion == 2;
    if (!(epsilon != 0.0)) epsilon = sqrt((double)P + 8 * sqrt((double)P)) * sigma;              // :413
    SBTV_TRY(upload_par(ctx, par, {mu1, mu2, 1.0 / mu1, 0.0}));
    run.numAt = 1;                                                       // ATy (:301)
    ctx->calls += 2;                                                     // AT(y), invLS(ATy, mu1) (:301,310)
    SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, xbuf[0]));  // :378-393
    if (opts->initialization == 0) ctx->calls += 1;
    if (opts->initialization == 2) run.numAt += 1;                       // :385
    // u = bu = 0, so s = 0 ; v = bv = 0 (:402-408)
    SBTV_HIP(ctx, hipMemsetAsync(s, 0, sizeof(double) * C, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(bu, 0, sizeof(double) * C, ctx->stream));
    if (!spectral) {
        SBTV_HIP(ctx, hipMemsetAsync(v, 0, sizeof(double) * P, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(bv, 0, sizeof(double) * P, ctx->stream));
    }
    // state before the loop (:416-448): criterion(1) = distance1(1) = ||Bx - y||, objective(1) = ||W'x||_1, distance2(1) =
    // ||W'x - u|| with u = 0 (wav_init_kernel against the zero array s), mses(1)
    const double *hs = nullptr;
    {
        SBTV_TRY(wav_analysis(ctx, wp, xbuf[0], w, 1));                  // :402
        SBTV_TRY(op_resid(ctx, c, xbuf[0], acc));                        // :416,444
        run.numA += 2;                                                   // :421,445
        ctx->calls += 2;
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));
        hipLaunchKernelGGL(wav_init_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)w, (const double *)s, partials, C);
        RedJobs jb;
        jb.add(acc, 1, nrb, sums);
        jb.add(partials, 2, nb, sums + 2);
        if (td) {
            hipLaunchKernelGGL(ad_xsums_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)xbuf[0], td,
                               (const double *)nullptr, ppix, P);
            jb.add(ppix, 3, nbp, sums + 4);
        }
        SBTV_TRY(reduce_jobs(ctx, jb));
        SBTV_HIP(ctx, hipGetLastError());
        SBTV_TRY(run.fetch(sums, 8, &hs));
        const double r0 = sqrt(hs[0] * c.parseval);
        if (criterion) criterion[0] = r0;                                // :446
        if (distance1) distance1[0] = r0;                                // :447, v = 0
        if (distance2) distance2[0] = sqrt(hs[3]);                       // :448
        if (objective) objective[0] = hs[2];                             // :423 with Phi = ||W'.||_1
        if (mses && td) mses[0] = hs[4] / (double)P;                     // :436
        if (times) times[0] = 0.0;
    }
    double crit_prev = sqrt(hs[0] * c.parseval), obj_prev = hs[2];
    if (spectral) {
        // v = bv = 0 before the loop: E = 0, s_prev = 1
        const double h[8] = {mu2, mu2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        SBTV_HIP(ctx, hipMemsetAsync(Es, 0, sizeof(double2) * c.fp.u_img, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(cst, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    SBTV_TRY(run.start());
    // a continuation factor changes the threshold every iteration: the host finishes an iteration before it enqueues the next
    const int lag = (delta == 1.0 && (opts->speculate & 1)) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {                               // :461
        const int k = outer - 1;
        double *xn = xbuf[k & 1];
        const double *xprev = xbuf[(k & 1) ^ 1];
        const double T = 1.0 / mu1;                                      // :463
        RedJobs jb;
        SBTV_TRY(wav_synthesis(ctx, wp, s, z, 1));                       // P(u + bu) (:467)
        if (spectral) {
            RowsArgs a{};
            a.dir_fwd = 1;
            a.dir_inv = 1;
            a.op = OP_CSALSA;
            a.H = c.Hs;
            a.Y = c.Ys;
            a.E = Es;
            a.cs = cst;
            a.mu = par;                                                  // mu1
            a.acc = acc;
            SBTV_TRY(fft_cols_fwd(ctx, c.fp, z, nullptr, c.S));
            SBTV_TRY(fft_rows(ctx, c.fp, c.S, c.S, a));                  // :467-471, 481-491
            SBTV_TRY(fft_cols_inv(ctx, c.fp, c.S, xn, c.inv_scale));
            hipLaunchKernelGGL(csalsa_scal_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double *)acc, nrb, cst, epsilon,
                               c.parseval, sums);
        } else {
            // r = mu1 P(u+bu) + mu2 AT(y+v+bv) ; x = invLS(r, mu1) (:467-471): X = (conj(H) fft2(mu2 (y+v+bv)) + mu1 fft2(z)) / (|H|^2 + mu1)
            hipLaunchKernelGGL(csalsa_w_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, yd, (const double *)v, (const double *)bv,
                               (const double *)par, wi, P);
            SBTV_TRY(op_spectrum(ctx, c.fp, wi, nullptr, c.S, Ws));
            SBTV_TRY(op_solve(ctx, c, z, nullptr, Ws, par, acc, xn));  // mu1; the residual sum in acc is not used here
        }
        SBTV_TRY(wav_analysis(ctx, wp, xn, w, 1));                       // :473
        hipLaunchKernelGGL(wav_cstep_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)w, bu, s, T, partials, C);   // :478, 492
        jb.add(partials, 2, nb, sums + 2);
        if (!spectral) {
            SBTV_TRY(op_apply(ctx, c, OP_MUL_H, xn, Ax));                // :481
            hipLaunchKernelGGL(csalsa_ve_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)Ax, yd, (const double *)bv,
                               pve, P);
            SBTV_TRY(reduce_partials(ctx, pve, 1, nbp, sums + 8));
            hipLaunchKernelGGL(csalsa_split_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)Ax, yd, v, bv,
                               (const double *)(sums + 8), epsilon, psplit, P);   // :483-491
            jb.add(psplit, 2, nbp, sums);
        }
        if (td || rule2) {
            hipLaunchKernelGGL(ad_xsums_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)xn, td,
                               rule2 ? xprev : (const double *)nullptr, ppix, P);
            jb.add(ppix, 3, nbp, sums + 4);
        }
        SBTV_TRY(reduce_jobs(ctx, jb));
        return run.publish(outer, sums, 8, 0);
    };
    bool stop = false;
    // host side of iteration `outer`: traces (:494-501) and the stop rule (:517-541)
    auto process = [&](int outer) -> int {
        const int k = outer - 1;                                         // the traces start at the first iteration
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        run.numAt += 1;
        run.numA += 1;
        ctx->calls += 3;                                                 // AT, invLS, A
        const double crit = sqrt(hsl[0]), obj = hsl[2];
        if (criterion) criterion[k] = crit;                              // :494
        if (distance1) distance1[k] = sqrt(hsl[1]);                      // :495
        if (distance2) distance2[k] = sqrt(hsl[3]);                      // :497
        if (objective) objective[k] = obj;                               // :498 with Phi = ||W'.||_1
        if (mses && td) mses[k] = hsl[4] / (double)P;                    // :501
        if (times) times[k] = run.seconds();
        if (delta != 1.0) {                                              // :517-518
            mu1 *= delta;
            mu2 *= delta;
            SBTV_TRY(upload_par(ctx, par, {mu1, mu2, 1.0 / mu1, 0.0}));
        }
        double sc;
        if (opts->stopcriterion == 1)
            sc = fabs(obj - obj_prev) / obj;                             // :527
        else if (opts->stopcriterion == 2)
            sc = fabs(sqrt(hsl[5]) / sqrt(hsl[6]));                      // :534
        else
            sc = fabs(crit - crit_prev) / crit;                          // :539
        obj_prev = obj;
        crit_prev = crit;
        stop = (sc < opts->tolA && crit <= epsilon);                     // :529,535,541
        return 0;
    };
    int last = 1;                                                        // the state before the loop is iteration 1 (:416-448)
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[(last - 1) & 1], x_out_dev);
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_CSALSA_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                        const double *h, int hlen, int levels, const double *mu1, const double *mu2, const double *sigma,
                        const double *epsilon, double continuationfactor, const sbtv_salsa_opts *opts, const double *true_x,
                        const double *x_init, double *x_out, double *objective, double *distance1, double *distance2,
                        double *criterion, double *times, double *mses, int *numA, int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "CSALSA_wavelet", y, taps, opts, x_init, M, N, batch, taille, "x_init", false));   // no TV prox
    if (!mu1 || !mu2 || !sigma || !x_out) return fail(ctx, SBTV_ERR_BADARG, "CSALSA_wavelet: missing required argument");
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0))
            return fail(ctx, SBTV_ERR_MISSING_LS, "(A^T A + \\mu I)^(-1) must be specified: mu1, mu2 must be > 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    // no sharded form: the arrays are staged and the images solved one after another
    const size_t P = (size_t)M * N, cnt = P * batch, t2 = (size_t)taille * taille;
    const double *yd = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "admm.in.true", true_x, cnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "admm.in.xinit", x_init, cnt, flags, &xi));
    double *xo = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, cnt, flags, &xo));
    for (size_t b = 0; b < (size_t)batch; ++b) {
        const size_t o = b * P, r = b * (size_t)opts->maxiter;           // every trace row has maxiter entries
        SBTV_TRY(csalsa_wavelet_one(ctx, yd + o, M, N, taps + b * t2, taille, wp, mu1[b], mu2[b], sigma[b],
                                    epsilon ? epsilon[b] : 0.0, continuationfactor, opts, off(td, o), off(xi, o), xo + o,
                                    off(objective, r), off(distance1, r), off(distance2, r), off(criterion, r), off(times, r),
                                    off(mses, r), off(numA, b), off(numAt, b), off(n_outer, b)));
    }
    SBTV_TRY(stage_out_copy(ctx, x_out, xo, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

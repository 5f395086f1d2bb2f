// The two other ADMM front-ends of the SALSA toolbox that call the Chambolle TV prox, built from
// the same device kernels as SALSA_v2:
//   C-SALSA  (SALSA/CSALSA_v2.m:160-561)  min TV(x)  s.t. ||Ax - y|| <= epsilon
//   CoRAL    (SALSA/CoRAL_v2.m:2-476)     min 0.5||Ax-y||^2 + tau1 TV(x) + tau2 TV(x)   (two split copies)
// and the masked-observation SALSA (no counterpart in the reference: SALSA/SALSA.m:103-104,308-312,463-464 takes a mask OR a
// blur), min 0.5 sum(m .* (Bx - y).^2) + tau TV(x) with the splits u = x and v = Bx (masked_one below).
// Neither is called by the reference's demos, so they are not fused to the last pass; what they share with the SALSA
// loop since round 3 is its stream discipline: the Chambolle launches of an outer iteration are OPTIMISTIC (all TViters
// iterations back to back, no stop-rule kernels, no redo pass; the host applies chambolle_prox_TV_stop.m:131 to the step
// sums it reads with the iteration's scalars and, should the rule ever fire before the last step, repeats the solve with
// exact launches), and the host evaluates the outer stop rule one iteration late while the next iteration already runs
// (x is double-buffered, so the result of the stopping iteration is intact).  The images of a batch are solved one after
// another.  What a pipelined single-image solve carries (AdmmRun) and the helpers of the element-wise kernels are in
// admm_run.inc, shared with the wavelet-l1 solvers of wavelet_deconv.hip, which run the same loop without the TV prox.
#include <chrono>
#include <cmath>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

#include "admm_run.inc"   // AB, ad_store_partials, AD_LOOP / AD_LD / AD_ST, ad_sub_kernel, ad_blocks, admm_common, upload_par, AdmmRun

// ---- C-SALSA -----------------------------------------------------------------------------------
#include "csalsa_step.inc"  // csalsa_w_kernel, csalsa_ve_kernel, csalsa_scal_kernel, csalsa_spectral_wanted

// projection of ve on the epsilon ball, multiplier updates and the sums of the traces (:483-501,534)
//   partials [6][nb]: (Ax-y)^2, (Ax-y-v)^2, (x-u)^2, (x-true)^2, (x-xprev)^2, x^2
__global__ __launch_bounds__(AB) void csalsa_update_kernel(const double *__restrict__ Ax, const double *__restrict__ y,
                                                            const double *__restrict__ x, const double *__restrict__ u,
                                                            double *__restrict__ v, double *__restrict__ bv,
                                                            double *__restrict__ bu, const double *__restrict__ tru,
                                                            const double *__restrict__ xprev,
                                                            const double *__restrict__ nve2, double eps,
                                                            double *__restrict__ partials, size_t P) {
    const double n_ve = sqrt(nve2[0]);
    const bool inside = n_ve <= eps;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    AD_LOOP(q, P) {
        const double2 a = AD_LD(Ax, q), yy = AD_LD(y, q), c = AD_LD(bv, q);
        const double t0 = a.x - yy.x, t1 = a.y - yy.y;
        const double e0 = t0 - c.x, e1 = t1 - c.y;
        const double v0 = inside ? e0 : e0 / n_ve * eps, v1 = inside ? e1 : e1 / n_ve * eps;
        AD_ST(v, q, make_double2(v0, v1));
        const double r0 = t0 - v0, r1 = t1 - v1;
        AD_ST(bv, q, make_double2(c.x - r0, c.y - r1));
        const double2 xv = AD_LD(x, q), uv = AD_LD(u, q), bb = AD_LD(bu, q);
        const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
        AD_ST(bu, q, make_double2(bb.x - d0, bb.y - d1));
        acc[0] += t0 * t0 + t1 * t1;
        acc[1] += r0 * r0 + r1 * r1;
        acc[2] += d0 * d0 + d1 * d1;
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[3] += m0 * m0 + m1 * m1;
        }
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[4] += m0 * m0 + m1 * m1;
        }
        acc[5] += xv.x * xv.x + xv.y * xv.y;
    }
    ad_store_partials<6>(acc, partials);
}

// after the prox of the spectral form (csalsa_scal_kernel, csalsa_step.inc): bu <- bu - (x - u) (:492) and the sums of the traces that live in the image domain
//   partials [5][nb]: (x-u)^2, (x-true)^2, (x-xprev)^2, x^2, periodic TV(x) (utils/TVnorm.m:2)
__global__ __launch_bounds__(AB) void csalsa_post_kernel(const double *__restrict__ x, const double *__restrict__ u,
                                                          double *__restrict__ bu, const double *__restrict__ tru,
                                                          const double *__restrict__ xprev, double *__restrict__ partials,
                                                          unsigned M, unsigned N, size_t P) {
    double acc[5] = {0, 0, 0, 0, 0};
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), uv = AD_LD(u, q), bb = AD_LD(bu, q);
        const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
        AD_ST(bu, q, make_double2(bb.x - d0, bb.y - d1));
        acc[0] += d0 * d0 + d1 * d1;
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[1] += m0 * m0 + m1 * m1;
        }
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[2] += m0 * m0 + m1 * m1;
        }
        acc[3] += xv.x * xv.x + xv.y * xv.y;
        // element 2q = (i, j), i even (M is even on this path): left neighbours in column j-1, upper neighbour of row i
        const unsigned idx = (unsigned)(2 * q), j = idx / M, i = idx - j * M;
        const size_t lcol = (size_t)(j > 0 ? j - 1 : N - 1) * M + i;
        const double2 xl = *reinterpret_cast<const double2 *>(x + lcol);
        const double xu = x[(size_t)j * M + (i > 0 ? i - 1 : M - 1)];
        const double h0 = xv.x - xl.x, v0 = xv.x - xu, h1 = xv.y - xl.y, v1 = xv.y - xv.x;
        acc[4] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
    }
    ad_store_partials<5>(acc, partials);
}

// ---- CoRAL -------------------------------------------------------------------------------------
// s = (mu1 (u+bu) + mu2 (v+bv)) / mu_ls                                     (CoRAL_v2.m:411, ATy enters spectrally)
// TVS: also the periodic TV norms of u and v (utils/TVnorm.m:2) for the objective (:425), partials [2][nb]: the two
// arrays are in flight here anyway (M even; element 2q = (i, j) with i even)
template <bool TVS>
__global__ __launch_bounds__(AB) void coral_s_kernel(const double *__restrict__ u, const double *__restrict__ bu,
                                                      const double *__restrict__ v, const double *__restrict__ bv,
                                                      double mu1, double mu2, double mu_ls, double *__restrict__ s,
                                                      double *__restrict__ partials, unsigned M, unsigned N, size_t P) {
    double acc[2] = {0, 0};
    AD_LOOP(q, P) {
        const double2 a = AD_LD(u, q), b = AD_LD(bu, q), c = AD_LD(v, q), d = AD_LD(bv, q);
        AD_ST(s, q, make_double2((mu1 * (a.x + b.x) + mu2 * (c.x + d.x)) / mu_ls,
                                 (mu1 * (a.y + b.y) + mu2 * (c.y + d.y)) / mu_ls));
        if constexpr (TVS) {
            const unsigned idx = (unsigned)(2 * q), j = idx / M, i = idx - j * M;
            const size_t lcol = (size_t)(j > 0 ? j - 1 : N - 1) * M + i, up = (size_t)j * M + (i > 0 ? i - 1 : M - 1);
            const double2 ul = *reinterpret_cast<const double2 *>(u + lcol), vl = *reinterpret_cast<const double2 *>(v + lcol);
            const double uu = u[up], vu = v[up];
            {
                const double h0 = a.x - ul.x, v0 = a.x - uu, h1 = a.y - ul.y, v1 = a.y - a.x;
                acc[0] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
            }
            {
                const double h0 = c.x - vl.x, v0 = c.x - vu, h1 = c.y - vl.y, v1 = c.y - c.x;
                acc[1] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
            }
        }
    }
    if constexpr (TVS) ad_store_partials<2>(acc, partials);
}

// bu += u - x ; bv += v - x ; g1 = x - bu ; g2 = x - bv  (:420-421 and the next prox inputs :401,406)
//   partials [7][nb]: (x-true)^2, (x-u)^2, (x-v)^2, x^2, u^2, v^2, (x-xprev)^2
__global__ __launch_bounds__(AB) void coral_post_kernel(const double *__restrict__ x, const double *__restrict__ xprev,
                                                         const double *__restrict__ u, const double *__restrict__ v,
                                                         double *__restrict__ bu, double *__restrict__ bv,
                                                         double *__restrict__ g1, double *__restrict__ g2,
                                                         const double *__restrict__ tru, double *__restrict__ partials,
                                                         size_t P) {
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), uv = AD_LD(u, q), vv = AD_LD(v, q);
        double2 b1 = AD_LD(bu, q), b2 = AD_LD(bv, q);
        b1.x = b1.x + (uv.x - xv.x);
        b1.y = b1.y + (uv.y - xv.y);
        b2.x = b2.x + (vv.x - xv.x);
        b2.y = b2.y + (vv.y - xv.y);
        AD_ST(bu, q, b1);
        AD_ST(bv, q, b2);
        AD_ST(g1, q, make_double2(xv.x - b1.x, xv.y - b1.y));
        AD_ST(g2, q, make_double2(xv.x - b2.x, xv.y - b2.y));
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[0] += m0 * m0 + m1 * m1;
        }
        {
            const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
            acc[1] += d0 * d0 + d1 * d1;
            const double e0 = xv.x - vv.x, e1 = xv.y - vv.y;
            acc[2] += e0 * e0 + e1 * e1;
        }
        acc[3] += xv.x * xv.x + xv.y * xv.y;
        acc[4] += uv.x * uv.x + uv.y * uv.y;
        acc[5] += vv.x * vv.x + vv.y * vv.y;
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[6] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<7>(acc, partials);
}

// ---- masked-observation SALSA (masked_one) ------------------------------------------------------
#include "masked_my.inc"  // masked_my_kernel: w = m .* y, shared with masked_wavelet.hip

// The one element-wise pass of an outer iteration, after the two inverse transforms (x, Bx) and with this iteration's u and v:
//   bu += u - x ; bv += v - Bx ; g = x - bu (the next prox input) ; v <- (m .* y + mu2 (Bx - bv)) ./ (m + mu2) (the next v)
//   partials [9 or 10][nb]: m (Bx-y)^2, (x-u)^2, (Bx-v)^2, x^2, u^2, Bx^2, v^2, (x-true)^2, (x-xprev)^2 and, TVS, the periodic
//   TV norm of u (utils/TVnorm.m:2; M even, element 2q = (i, j) with i even), all with the v this iteration solved with
template <bool TVS>
__global__ __launch_bounds__(AB) void masked_post_kernel(const double *__restrict__ x, const double *__restrict__ xprev,
                                                          const double *__restrict__ Bx, const double *__restrict__ u,
                                                          const double *__restrict__ y, const double *__restrict__ m,
                                                          double *__restrict__ bu, double *__restrict__ v,
                                                          double *__restrict__ bv, double *__restrict__ g,
                                                          const double *__restrict__ tru, double mu2,
                                                          double *__restrict__ partials, unsigned M, unsigned N, size_t P) {
    constexpr int NQ = TVS ? 10 : 9;
    double acc[NQ];
#pragma unroll
    for (int c = 0; c < NQ; ++c) acc[c] = 0.0;
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), ax = AD_LD(Bx, q), uv = AD_LD(u, q), vv = AD_LD(v, q);
        const double2 yv = AD_LD(y, q), mv = AD_LD(m, q);
        double2 b1 = AD_LD(bu, q), b2 = AD_LD(bv, q);
        b1.x = b1.x + (uv.x - xv.x);
        b1.y = b1.y + (uv.y - xv.y);
        b2.x = b2.x + (vv.x - ax.x);
        b2.y = b2.y + (vv.y - ax.y);
        AD_ST(bu, q, b1);
        AD_ST(bv, q, b2);
        AD_ST(g, q, make_double2(xv.x - b1.x, xv.y - b1.y));
        AD_ST(v, q, make_double2((mv.x * yv.x + mu2 * (ax.x - b2.x)) / (mv.x + mu2),
                                 (mv.y * yv.y + mu2 * (ax.y - b2.y)) / (mv.y + mu2)));
        {
            const double e0 = ax.x - yv.x, e1 = ax.y - yv.y;
            acc[0] += mv.x * (e0 * e0) + mv.y * (e1 * e1);
            const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
            acc[1] += d0 * d0 + d1 * d1;
            const double r0 = ax.x - vv.x, r1 = ax.y - vv.y;
            acc[2] += r0 * r0 + r1 * r1;
        }
        acc[3] += xv.x * xv.x + xv.y * xv.y;
        acc[4] += uv.x * uv.x + uv.y * uv.y;
        acc[5] += ax.x * ax.x + ax.y * ax.y;
        acc[6] += vv.x * vv.x + vv.y * vv.y;
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[7] += m0 * m0 + m1 * m1;
        }
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[8] += m0 * m0 + m1 * m1;
        }
        if constexpr (TVS) {
            const unsigned idx = (unsigned)(2 * q), j = idx / M, i = idx - j * M;
            const size_t lcol = (size_t)(j > 0 ? j - 1 : N - 1) * M + i;
            const double2 ul = *reinterpret_cast<const double2 *>(u + lcol);
            const double uu = u[(size_t)j * M + (i > 0 ? i - 1 : M - 1)];
            const double h0 = uv.x - ul.x, v0 = uv.x - uu, h1 = uv.y - ul.y, v1 = uv.y - uv.x;
            acc[NQ - 1] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
        }
    }
    ad_store_partials<NQ>(acc, partials);
}

#include "admm_prox.inc"  // AdmmProx: the warm-started TV prox of an outer iteration, optimistic or exact launches

// ------------------------------------------------------------------------------------------------
int csalsa_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, double mu1, double mu2,
               double sigma, double epsilon, double delta, const sbtv_salsa_opts *opts, const double *td,
               const double *xi, double *x_out_dev, double *objective, double *distance1, double *distance2,
               double *criterion, double *times, double *mses, int *numA, int *numAt, int *n_outer, bool spec_wanted) {
    BlurOp c;
    bool spectral = false;
    {
        FftPlan chk;
        SBTV_TRY(fft_plan(ctx, M, N, 1, &chk));
        // spectral form of the constraint split (see `enqueue_spectral` below): needs fixed mu1 / mu2, an even M (pairs of
        // one column per lane) and the row kernels that carry OP_CSALSA
        const bool sp = delta == 1.0 && csalsa_spectral_wanted() && fft_rows_csalsa_ok(chk) && !(M & 1) &&
                        (size_t)M * N < ((size_t)1 << 31);
        SBTV_TRY(admm_common(ctx, M, N, taps, taille, sp ? yd : nullptr, &c));
        spectral = sp;
    }
    const int K = opts->TViters;
    AdmmProx prox;
    SBTV_TRY(prox.plan(ctx, M, N, 1, "prox", K, opts));
    const size_t P = c.P;
    const int nb = ad_blocks(P);
    double *xbuf[2], *u, *bu, *v, *bv, *w, *Ax, *g, *par, *partials, *sums, *acc;
    double2 *Ws;
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * fft_rows_blocks(c.fp), &acc));
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &u));
    SBTV_TRY(ws_get_t(ctx, "admm.bu", P, &bu));
    SBTV_TRY(ws_get_t(ctx, "admm.v", P, &v));
    SBTV_TRY(ws_get_t(ctx, "admm.bv", P, &bv));
    SBTV_TRY(ws_get_t(ctx, "admm.w", P, &w));
    SBTV_TRY(ws_get_t(ctx, "admm.Ax", P, &Ax));
    SBTV_TRY(ws_get_t(ctx, "admm.g", P, &g));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu1, mu2, 1/mu1
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)8 * nb, &partials));
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)64, &sums));            // [0..5] update sums, [6] TV(x), [8] n_ve^2, [16..] prox step sums
    SBTV_TRY(ws_get_t(ctx, "admm.W", c.fp.u_img, &Ws));
    double2 *Es = Ws;                                                   // spectral form: the state spectrum E (W is not formed)
    double *cst = nullptr, *rs = nullptr;
    SBTV_TRY(ws_get_t(ctx, "admm.cs", (size_t)8, &cst));
    SBTV_TRY(ws_get_t(ctx, "admm.rs", (size_t)4, &rs));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    const double *hs = nullptr;
    const int maxiter = opts->maxiter;
    if (!(epsilon != 0.0)) epsilon = sqrt((double)P + 8 * sqrt((double)P)) * sigma;              // :413
    SBTV_TRY(upload_par(ctx, par, {mu1, mu2, 1.0 / mu1, 0.0}));
    run.numAt = 1;                                                       // ATy (:301)
    ctx->calls += 2;                                                     // AT(y), invLS(ATy, mu1) (:301,310)
    double *x = xbuf[0];
    SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, x));
    if (opts->initialization == 0) ctx->calls += 1;
    if (opts->initialization == 2) run.numAt += 1;                       // :385
    SBTV_HIP(ctx, hipMemsetAsync(u, 0, sizeof(double) * P, ctx->stream));   // :404-408
    SBTV_HIP(ctx, hipMemsetAsync(bu, 0, sizeof(double) * P, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(v, 0, sizeof(double) * P, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(bv, 0, sizeof(double) * P, ctx->stream));
    prox.lam = par + 2;                                                  // 1 / mu1
    SBTV_TRY(prox_zero_duals(ctx, prox.pp));                             // :440-441
    SBTV_TRY(prox.arm(ctx, true));

    // state before the loop (:416-448): Ax, criterion(1), objective(1) = TV(x), mses(1), distances
    SBTV_TRY(op_apply(ctx, c, OP_MUL_H, x, Ax));
    run.numA += 2;                                                       // :421,445
    ctx->calls += 2;
    {
        // v = 0, bv = 0, u = 0: the update kernel on scratch multipliers gives the three norms without side effects
        double *sv, *sbv, *sbu;
        SBTV_TRY(ws_get_t(ctx, "admm.scratch0", P, &sv));
        SBTV_TRY(ws_get_t(ctx, "admm.scratch1", P, &sbv));
        SBTV_TRY(ws_get_t(ctx, "admm.scratch2", P, &sbu));
        SBTV_HIP(ctx, hipMemsetAsync(sbv, 0, sizeof(double) * P, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(sbu, 0, sizeof(double) * P, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));   // n_ve^2 = 0 -> inside the ball, v = ve
        hipLaunchKernelGGL(csalsa_update_kernel, dim3(nb), dim3(AB), 0, ctx->stream, Ax, yd, x, u, sv, sbv, sbu, td,
                           (const double *)nullptr, sums + 8, 1.0, partials, P);
        SBTV_TRY(reduce_partials(ctx, partials, 6, nb, sums));
        SBTV_TRY(tvnorm_dev(ctx, x, M, N, 1, sums + 6));
        SBTV_TRY(run.fetch(sums, 8, &hs));
        // before the loop v = 0, so distance1(1) = ||Ax-y-v|| = ||Ax-y|| (:447); hs[1] is not that (v=ve there)
        if (criterion) criterion[0] = sqrt(hs[0]);
        if (distance1) distance1[0] = sqrt(hs[0]);
        if (distance2) distance2[0] = sqrt(hs[2]);                       // ||x - u||, u = 0 (:448)
        if (objective) objective[0] = hs[6];                             // phi(x) = TVnorm(x) (:423)
        if (mses && td) mses[0] = hs[3] / (double)P;                     // :436
        if (times) times[0] = 0.0;
    }
    double crit_prev = sqrt(hs[0]), obj_prev = hs[6];
    SBTV_TRY(run.start());
    // optimistic prox launches need a fixed threshold (the control block is armed once) and the tile kernels
    const bool spec = spec_wanted && delta == 1.0 && prox_spec_ok(prox.pp, g, u, K);
    const int lag = (spec && (opts->speculate & 1)) ? 1 : 0;
    // end of an enqueue: the sums (with the step sums of an optimistic prox) or the iteration count of an exact prox
    auto publish = [&](int outer) {
        return run.publish(outer, sums, 16 + (spec ? K : 0), spec ? K : 0, spec ? nullptr : prox.pp.ctrl);
    };
    const bool tv_fused = fft_cols_tv_ok(c.fp);
    const int ntv = tv_fused ? fft_cols_blocks(c.fp) : 0;
    double *tvp = nullptr;
    if (tv_fused) SBTV_TRY(ws_get_t(ctx, "admm.tvc", (size_t)ntv, &tvp));
    if (spectral) {
        // v = bv = 0 before the loop: E = 0, s_prev = 1
        const double h[8] = {mu2, mu2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        SBTV_HIP(ctx, hipMemsetAsync(Es, 0, sizeof(double2) * c.fp.u_img, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(cst, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    // Spectral form of an outer iteration.  The projection on the epsilon ball scales ve = Ax - y - bv by ONE scalar
    // s = min(1, eps/||ve||) (:485-489), so v = s ve, bv' = bv - (Ax - y - v) = -(1 - s) ve, and the next right-hand side
    // y + v + bv' = y + (2s - 1) ve: the split (v, bv) is the spectrum E of ve and the scalar s.  One row pass then does
    // what took three transforms: W = mu2 (Y + (2 s_prev - 1) E), X = (conj(H) W + mu1 S)/(|H|^2 + mu1), T = H X - Y
    // (= fft2(Ax - y)), E' = T + (1 - s_prev) E, with ||Ax-y||^2, ||ve||^2 and ||E' - E||^2 by Parseval (the norms the
    // traces and the next s need).  Image-domain work left: u + bu into the forward pass, x - bu for the prox, and one
    // pass for bu, TV(x) and the sums over x.
    auto enqueue_spectral = [&](int outer) -> int {
        const int k = outer - 1;
        double *xn = xbuf[k & 1];
        const double *xprev = xbuf[(k & 1) ^ 1];
        RowsArgs a{};
        a.dir_fwd = 1;
        a.dir_inv = 1;
        a.op = OP_CSALSA;
        a.H = c.Hs;
        a.Y = c.Ys;
        a.E = Es;
        a.cs = cst;
        a.mu = par;                                                      // mu1
        a.acc = acc;
        SBTV_TRY(fft_cols_fwd(ctx, c.fp, u, bu, c.S));
        SBTV_TRY(fft_rows(ctx, c.fp, c.S, c.S, a));
        if (fft_cols_inv_step_ok(c.fp)) {
            SBTV_TRY(fft_cols_inv_sub(ctx, c.fp, c.S, xn, c.inv_scale, bu, g));       // x and the prox input x - bu
        } else {
            SBTV_TRY(fft_cols_inv(ctx, c.fp, c.S, xn, c.inv_scale));
            hipLaunchKernelGGL(ad_sub_kernel, dim3(nb), dim3(AB), 0, ctx->stream, xn, bu, g, P);
        }
        hipLaunchKernelGGL(csalsa_scal_kernel, dim3(1), dim3(256), 0, ctx->stream, acc, fft_rows_blocks(c.fp), cst, epsilon,
                           c.parseval, sums);
        RedJobs jb;
        SBTV_TRY(prox.run(ctx, g, u, spec, sums + 16, &jb));             // step sums: reduced with the sums of the last pass
        hipLaunchKernelGGL(csalsa_post_kernel, dim3(nb), dim3(AB), 0, ctx->stream, xn, u, bu, td,
                           (opts->stopcriterion == 2) ? xprev : (const double *)nullptr, partials, (unsigned)M, (unsigned)N, P);
        jb.add(partials, 5, nb, sums + 2);
        SBTV_TRY(reduce_jobs(ctx, jb));
        return publish(outer);
    };
    auto enqueue = [&](int outer) -> int {                               // :461
        if (spectral) return enqueue_spectral(outer);
        const int k = outer - 1;
        double *xn = xbuf[k & 1];
        const double *xprev = xbuf[(k & 1) ^ 1];
        // r = mu1 (u+bu) + mu2 AT(y+v+bv) ; x = invLS(r, mu1)   (:467-471), all in one spectral pass:
        //   X = (conj(H) W + mu1 S) / (|H|^2 + mu1),  W = fft2(mu2 (y+v+bv)),  S = fft2(u+bu)
        hipLaunchKernelGGL(csalsa_w_kernel, dim3(nb), dim3(AB), 0, ctx->stream, yd, v, bv, par, w, P);
        SBTV_TRY(op_spectrum(ctx, c.fp, w, nullptr, c.S, Ws));
        SBTV_TRY(op_solve(ctx, c, u, bu, Ws, par, acc, xn));           // mu1; the residual sum in acc is not used here
        // u = prox_{TV/mu1}(x - bu), warm-started duals (:476)
        hipLaunchKernelGGL(ad_sub_kernel, dim3(nb), dim3(AB), 0, ctx->stream, xn, bu, g, P);
        SBTV_TRY(prox.run(ctx, g, u, spec, sums + 16, nullptr));
        // Ax (the forward column pass of x also leaves the periodic-TV partials of phi(x) = TVnorm(x), :498), projection on
        // the epsilon ball, multipliers, traces (:481-501)
        {
            RowsArgs a{};
            a.dir_fwd = 1;
            a.dir_inv = 1;
            a.op = OP_MUL_H;
            a.H = c.Hs;
            SBTV_TRY(fft_cols_fwd_f(ctx, c.fp, xn, nullptr, c.S, nullptr, tvp));
            SBTV_TRY(fft_rows(ctx, c.fp, c.S, c.S, a));
            SBTV_TRY(fft_cols_inv(ctx, c.fp, c.S, Ax, c.inv_scale));
        }
        hipLaunchKernelGGL(csalsa_ve_kernel, dim3(nb), dim3(AB), 0, ctx->stream, Ax, yd, bv, partials, P);
        SBTV_TRY(reduce_partials(ctx, partials, 1, nb, sums + 8));
        hipLaunchKernelGGL(csalsa_update_kernel, dim3(nb), dim3(AB), 0, ctx->stream, Ax, yd, xn, u, v, bv, bu, td,
                           (opts->stopcriterion == 2) ? xprev : (const double *)nullptr, sums + 8, epsilon, partials, P);
        SBTV_TRY(reduce_partials(ctx, partials, 6, nb, sums));
        if (tv_fused) SBTV_TRY(reduce_partials(ctx, tvp, 1, ntv, sums + 6));
        else SBTV_TRY(tvnorm_dev(ctx, xn, M, N, 1, sums + 6));
        return publish(outer);
    };
    bool stop = false;
    // host side of iteration `outer`: traces (:494-501) and the stop rule (:517-541)
    auto process = [&](int outer) -> int {
        const int k = outer - 1;                                         // the traces start at the first iteration
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        if (spec) SBTV_TRY(prox.check(ctx, hsl + 16));
        run.numAt += 1;
        run.numA += 1;
        ctx->calls += 3;                                                 // AT, invLS, A
        const double crit = sqrt(hsl[0]), obj = hsl[6];
        if (criterion) criterion[k] = crit;                              // :494
        if (distance1) distance1[k] = sqrt(hsl[1]);                      // :495
        if (distance2) distance2[k] = sqrt(hsl[2]);                      // :497
        if (objective) objective[k] = obj;                               // :498
        if (mses && td) mses[k] = hsl[3] / (double)P;                    // :501
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
            sc = fabs(sqrt(hsl[4]) / sqrt(hsl[5]));                      // :534
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

// ------------------------------------------------------------------------------------------------
int coral_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, double tau1, double tau2,
              double mu1, double mu2, double mu_ls, int TViters2, const sbtv_salsa_opts *opts, const double *td,
              const double *xi, double *x_out_dev, double *objective, double *distance, double *times, double *mses,
              int *numA, int *numAt, int *n_outer, bool spec_wanted) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, yd, &c));
    // The two TV proxes of an iteration are independent (:401,406).  With the same iteration count they run as ONE batch of
    // two images (own threshold, own duals, own stop rule per image: the batch semantics of the prox): two Chambolle
    // launches with twice the tiles per outer iteration instead of four (SBTV_CORAL_BATCH=0: one plan per prox)
    static const bool env_batch = [] {
        const char *e = getenv("SBTV_CORAL_BATCH");
        return !(e && e[0] == '0');
    }();
    const bool batched = env_batch && opts->TViters == TViters2;
    const int K1 = opts->TViters, K2 = TViters2;
    AdmmProx pu, pv;                                                     // batched: pu is the plan of both images
    SBTV_TRY(pu.plan(ctx, M, N, batched ? 2 : 1, batched ? "prox.pair" : "prox", K1, opts));
    if (!batched) SBTV_TRY(pv.plan(ctx, M, N, 1, "prox2", K2, opts));
    const size_t P = c.P;
    const int nb = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    const bool tv_in_s = !(M & 1) && P < ((size_t)1 << 31);             // TV(u), TV(v) ride in the pass that forms s
    double *xbuf[2], *u, *bu, *v, *bv, *s, *g1, *g2, *par, *partials, *sums, *acc, *tvpart;
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.uv", 2 * P, &u));                      // [u | v] and [g1 | g2]: the images of the batch
    v = u + P;
    SBTV_TRY(ws_get_t(ctx, "admm.bu", P, &bu));
    SBTV_TRY(ws_get_t(ctx, "admm.bv", P, &bv));
    SBTV_TRY(ws_get_t(ctx, "admm.w", P, &s));
    SBTV_TRY(ws_get_t(ctx, "admm.g12", 2 * P, &g1));
    g2 = g1 + P;
    SBTV_TRY(ws_get_t(ctx, "admm.tvpart", (size_t)2 * nb, &tvpart));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu_ls, thr1, thr2
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)8 * nb, &partials));
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));            // [0..6] post sums, [8] resid2, [9] TV(u), [10] TV(v), [16..], [48..] step sums
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    SBTV_TRY(upload_par(ctx, par, {mu_ls, tau1 / mu1, tau2 / mu2, 0.0}));   // thresholds :356,361
    pu.lam = par + 1;
    pv.lam = par + 2;
    const int maxiter = opts->maxiter;
    run.numAt = 2;                                                       // ATy twice (:189,219)
    ctx->calls += 3;                                                     // AT(y), invLS(ATy), AT(y)
    double *x = xbuf[0];
    SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, x));
    if (opts->initialization == 0) ctx->calls += 1;
    // u = x ; bu = u ; v = x ; bv = v  (:353-359)  ->  first prox inputs x - bu = x - bv = 0
    for (double *dst : {u, bu, v, bv})
        SBTV_HIP(ctx, hipMemcpyAsync(dst, x, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(g1, 0, sizeof(double) * P, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(g2, 0, sizeof(double) * P, ctx->stream));
    SBTV_TRY(prox_zero_duals(ctx, pu.pp));                               // :384-392
    SBTV_TRY(pu.arm(ctx, true));
    if (!batched) {
        SBTV_TRY(prox_zero_duals(ctx, pv.pp));
        SBTV_TRY(pv.arm(ctx, true));
    }

    // initial objective (:366-368)
    double obj_prev;
    {
        SBTV_TRY(op_resid(ctx, c, x, acc));
        SBTV_TRY(reduce_partials(ctx, acc, 1, nrb, sums + 8));
        SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 9));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 8, ctx->stream));
        if (td) {
            double *o4 = nullptr;
            SBTV_TRY(ws_get_t(ctx, "admm.o4", (size_t)4, &o4));
            SBTV_TRY(pair_sums(ctx, x, td, P, 1, o4));
            SBTV_HIP(ctx, hipMemcpyAsync(sums, o4, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        }
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        run.numA += 1;
        ctx->calls += 1;
        obj_prev = 0.5 * (hs[8] * c.parseval) + tau1 * hs[9] + tau2 * hs[9];   // u = v = x
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[0] / (double)P;                     // :381
    }
    SBTV_TRY(run.start());
    const bool spec = spec_wanted && prox_spec_ok(pu.pp, g1, u, K1) &&
                      (batched || prox_spec_ok(pv.pp, g2, v, K2));
    const int lag = (spec && (opts->speculate & 1)) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {                               // :394
        double *xn = xbuf[outer & 1];
        const double *xprev = xbuf[(outer & 1) ^ 1];
        // the two TV proxes with their own warm-started duals (:401,406).  The first outer iteration always runs exactly:
        // its prox inputs x - bu = x - bv are zero and the rule stops at k = 1; its control blocks are re-armed afterwards
        const bool sp = spec && outer >= 2;
        RedJobs jb;
        if (spec && outer == 2) {
            SBTV_TRY(pu.arm(ctx, false));
            if (!batched) SBTV_TRY(pv.arm(ctx, false));
        }
        if (batched) {
            // both images in one plan: the step sums of image b land at sums + 16 + b FSTRIDE (= sums + 48 for v), reduced
            // at the end of the iteration
            static_assert(FSTRIDE == 32, "the step sums of the second prox are read at sums + 48");
            SBTV_TRY(pu.run(ctx, g1, u, sp, sums + 16, &jb));
        } else {
            SBTV_TRY(pu.run(ctx, g1, u, sp, sums + 16, nullptr));
            SBTV_TRY(pv.run(ctx, g2, v, sp, sums + 48, nullptr));
        }
        // r = ATy + mu1 (u+bu) + mu2 (v+bv) ; x = invLS(r)   (:411-413)  + residual energy (:423, Parseval)
        if (tv_in_s) {
            hipLaunchKernelGGL(coral_s_kernel<true>, dim3(nb), dim3(AB), 0, ctx->stream, u, bu, v, bv, mu1, mu2, mu_ls, s, tvpart,
                               (unsigned)M, (unsigned)N, P);
            jb.add(tvpart, 2, nb, sums + 9);
        } else {
            hipLaunchKernelGGL(coral_s_kernel<false>, dim3(nb), dim3(AB), 0, ctx->stream, u, bu, v, bv, mu1, mu2, mu_ls, s, tvpart,
                               (unsigned)M, (unsigned)N, P);
        }
        SBTV_TRY(op_solve(ctx, c, s, nullptr, c.Ys, par, acc, xn));    // mu_ls
        hipLaunchKernelGGL(coral_post_kernel, dim3(nb), dim3(AB), 0, ctx->stream, xn,
                           (opts->stopcriterion == 2) ? xprev : (const double *)nullptr, u, v, bu, bv, g1, g2, td, partials, P);
        jb.add(partials, 7, nb, sums);
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        if (!tv_in_s) {
            SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 9));
            SBTV_TRY(tvnorm_dev(ctx, v, M, N, 1, sums + 10));
        }
        if (sp) return run.publish(outer, sums, 80, K1 + K2);
        return run.publish(outer, sums, 12, 0, pu.pp.ctrl, batched ? pu.pp.ctrl + 1 : pv.pp.ctrl);
    };
    bool stop = false;
    auto process = [&](int outer) -> int {
        const double *hsl;
        const bool sp = spec && outer >= 2;
        SBTV_TRY(run.wait(outer, &hsl));
        if (sp) {     // per plan: batched, the step sums of v are those of the plan's second image (sums + 48)
            SBTV_TRY(pu.check(ctx, hsl + 16));
            if (!batched) SBTV_TRY(pv.check(ctx, hsl + 48));
        }
        run.numA += 1;
        ctx->calls += 2;                                                 // invLS, A
        const double f = 0.5 * (hsl[8] * c.parseval) + tau1 * hsl[9] + tau2 * hsl[10];      // :425
        if (objective) objective[outer] = f;
        if (mses && td) mses[outer] = hsl[0] / (double)P;                // :428-429
        if (distance) {
            distance[(size_t)(outer - 1) * 2] = sqrt(hsl[1]) / sqrt(hsl[3] + hsl[4]);       // :432
            distance[(size_t)(outer - 1) * 2 + 1] = sqrt(hsl[2]) / sqrt(hsl[3] + hsl[5]);   // :433
        }
        if (times) times[outer] = run.seconds();
        stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[6], hsl[3], opts->tolA);
        obj_prev = f;
        return 0;
    };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[last & 1], x_out_dev);
}

// ------------------------------------------------------------------------------------------------
// Masked-observation SALSA:  min_x 0.5 sum(m .* (B x - y).^2) + tau TV(x)  with the splits u = x (TV) and v = B x (data),
// the ADMM of Almeida & Figueiredo (IEEE TIP 2013) in SALSA_v2's sign convention (include/sbtv.h states the iteration).
// The spectral solve with its two right-hand sides,
//     X = (mu1 fft2(u+bu) + mu2 conj(H) fft2(v+bv)) / (mu1 + mu2 |H|^2)
//       = (conj(H) W + r S) / (|H|^2 + r),   W = fft2(v+bv), S = fft2(u+bu), r = mu1 / mu2,
// is the row pass OP_SALSA with the per-iteration spectrum W in the place of fft2(y) and r in the place of mu: no new
// row kernel.  Bx needs no forward column pass either: the row pass leaves S = N colFFT(x) (the column-transformed x), so a
// second row pass with OP_MUL_H on that S and an inverse column pass scaled by 1/N more give real(ifft2(H X)).  Per outer
// iteration: 2 forward column passes (v+bv, u+bu), 3 row passes (+ the unpack of W), 2 inverse column passes, the prox,
// one element-wise pass and one reduction launch.
int masked_one(sbtv_ctx *ctx, const double *yd, const double *md, int M, int N, const double *taps, int taille, double tau,
               double mu1, double mu2, const sbtv_salsa_opts *opts, const double *td, const double *xi, double *x_out_dev,
               double *objective, double *distance, double *times, double *mses, int *numA, int *numAt, int *n_outer,
               bool spec_wanted) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, nullptr, &c));
    const int K = opts->TViters;
    AdmmProx prox;
    SBTV_TRY(prox.plan(ctx, M, N, 1, "prox", K, opts));
    const size_t P = c.P;
    const int nb = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    const bool tv_in_post = !(M & 1) && P < ((size_t)1 << 31);          // TV(u) rides in the element-wise pass
    const int nq = tv_in_post ? 10 : 9;
    double *xbuf[2], *u, *bu, *v, *bv, *Bx, *g, *par, *partials, *sums, *acc;
    double2 *Ws, *S2;
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &u));
    SBTV_TRY(ws_get_t(ctx, "admm.bu", P, &bu));
    SBTV_TRY(ws_get_t(ctx, "admm.v", P, &v));
    SBTV_TRY(ws_get_t(ctx, "admm.bv", P, &bv));
    SBTV_TRY(ws_get_t(ctx, "admm.Ax", P, &Bx));
    SBTV_TRY(ws_get_t(ctx, "admm.g", P, &g));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu1 / mu2, tau / mu1
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * nb, &partials));
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));            // [0..9] sums of the element-wise pass, [16..] prox step sums
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));         // residual sum of OP_SALSA (against W: not used)
    SBTV_TRY(ws_get_t(ctx, "admm.W", c.fp.u_img, &Ws));
    SBTV_TRY(ws_get_t(ctx, "admm.S2", c.fp.s_img, &S2));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    SBTV_TRY(upload_par(ctx, par, {mu1 / mu2, tau / mu1, 0.0, 0.0}));
    prox.lam = par + 1;
    // the inverse column pass of H X takes the spectrum the row pass of X left: N times the column transform of x (the
    // chirp-z path keeps whole 2-D spectra, its "row pass" is point-wise)
    const double bx_scale = c.fp.generic ? c.inv_scale : c.inv_scale / (double)N;
    auto post = [&](const double *xn, const double *xprev) {
        if (tv_in_post)
            hipLaunchKernelGGL(masked_post_kernel<true>, dim3(nb), dim3(AB), 0, ctx->stream, xn, xprev, (const double *)Bx,
                               (const double *)u, yd, md, bu, v, bv, g, td, mu2, partials, (unsigned)M, (unsigned)N, P);
        else
            hipLaunchKernelGGL(masked_post_kernel<false>, dim3(nb), dim3(AB), 0, ctx->stream, xn, xprev, (const double *)Bx,
                               (const double *)u, yd, md, bu, v, bv, g, td, mu2, partials, (unsigned)M, (unsigned)N, P);
    };
    const int maxiter = opts->maxiter;
    double *x = xbuf[0];
    if (opts->initialization == 2) {                                     // x = B'(m .* y)
        hipLaunchKernelGGL(masked_my_kernel, dim3(nb), dim3(AB), 0, ctx->stream, md, yd, g, P);
        SBTV_TRY(op_apply(ctx, c, OP_MUL_HC, g, x));
        run.numAt += 1;
        ctx->calls += 1;
    } else {
        SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, x));
    }
    // Bx = B x ; u = x ; v = Bx ; bu = bv = 0 ; zero duals.  The element-wise pass on that state leaves bu = bv = 0, the
    // first prox input g = x, the first v and the sums of objective(1) / mses(1)
    SBTV_TRY(op_apply(ctx, c, OP_MUL_H, x, Bx));
    run.numA += 1;
    ctx->calls += 1;
    SBTV_HIP(ctx, hipMemcpyAsync(u, x, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(v, Bx, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(bu, 0, sizeof(double) * P, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(bv, 0, sizeof(double) * P, ctx->stream));
    SBTV_TRY(prox_zero_duals(ctx, prox.pp));
    SBTV_TRY(prox.arm(ctx, true));
    double obj_prev;
    {
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));
        post(x, nullptr);
        SBTV_TRY(reduce_partials(ctx, partials, nq, nb, sums));
        if (!tv_in_post) SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 9));
        SBTV_HIP(ctx, hipGetLastError());
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        obj_prev = 0.5 * hs[0] + tau * hs[9];
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[7] / (double)P;
    }
    SBTV_TRY(run.start());
    const bool spec = spec_wanted && prox_spec_ok(prox.pp, g, u, K);
    const int lag = (spec && (opts->speculate & 1)) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {
        double *xn = xbuf[outer & 1];
        const double *xprev = xbuf[(outer & 1) ^ 1];
        // u = prox_{(tau/mu1) TV}(x - bu), warm-started duals.  The first outer iteration always runs exactly (a zero start
        // gives a zero prox input and the rule stops at k = 1); the control block is re-armed for the optimistic launches
        const bool sp = spec && outer >= 2;
        RedJobs jb;
        if (spec && outer == 2) SBTV_TRY(prox.arm(ctx, false));
        SBTV_TRY(prox.run(ctx, g, u, sp, sums + 16, &jb));               // step sums: reduced at the end of the iteration
        // W = fft2(v + bv) (v was formed by the previous element-wise pass)
        SBTV_TRY(op_spectrum(ctx, c.fp, v, bv, S2, Ws));
        // X = (conj(H) W + r fft2(u + bu)) / (|H|^2 + r), r = mu1 / mu2 ; x = real(ifft2(X))
        SBTV_TRY(op_solve(ctx, c, u, bu, Ws, par, acc, xn));
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
        post(xn, (opts->stopcriterion == 2) ? xprev : (const double *)nullptr);
        jb.add(partials, nq, nb, sums);
        SBTV_TRY(reduce_jobs(ctx, jb));
        if (!tv_in_post) SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 9));
        return run.publish(outer, sums, sp ? 16 + K : 12, sp ? K : 0, sp ? nullptr : prox.pp.ctrl);
    };
    bool stop = false;
    // host side of iteration `outer`: traces and the stop rule of SALSA_v2.m:442-482
    auto process = [&](int outer) -> int {
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        if (spec && outer >= 2) SBTV_TRY(prox.check(ctx, hsl + 16));
        run.numA += 1;                                                   // H .* X
        run.numAt += 1;                                                  // conj(H) .* fft2(v + bv)
        ctx->calls += 2;
        const double f = 0.5 * hsl[0] + tau * hsl[9];
        if (objective) objective[outer] = f;
        if (mses && td) mses[outer] = hsl[7] / (double)P;
        if (distance) {
            distance[(size_t)(outer - 1) * 2] = sqrt(hsl[1]) / sqrt(hsl[3] + hsl[4]);
            distance[(size_t)(outer - 1) * 2 + 1] = sqrt(hsl[2]) / sqrt(hsl[5] + hsl[6]);
        }
        if (times) times[outer] = run.seconds();
        stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[8], hsl[3], opts->tolA);
        obj_prev = f;
        return 0;
    };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[last & 1], x_out_dev);
}

// item b of a batch as its solver sees it (device pointers)
struct AdmmItem {
    const double *y, *mask, *tru, *x_init;
    double *x;
};

// What sbtv_CSALSA_v2, sbtv_CoRAL_v2 and sbtv_SALSA_masked do once their arguments are checked.  Independent images go to
// the lanes of this context (`sharded`, group.hip) when it has them.  Else the arrays are staged and the images solved one
// after another by one(b, item, spec): optimistic prox launches first (unless bit 1 of `speculate` asks for exact ones),
// exact ones if the rule fired early.
template <class Sharded, class One>
int admm_batch(sbtv_ctx *ctx, int M, int N, int batch, const sbtv_salsa_opts *opts, const double *y, const double *mask,
               const double *true_x, const double *x_init, double *x_out, int flags, Sharded &&sharded, One &&one) {
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    if (sbtv_group *lg = lanes_group(ctx, batch, false)) {
        LaneCall lc(ctx, lg);
        return lc.done(sharded(lg), batch);
    }
    const size_t P = (size_t)M * N, cnt = P * batch;
    const double *yd = nullptr, *md = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "admm.in.mask", mask, cnt, flags, &md));
    SBTV_TRY(stage_in(ctx, "admm.in.true", true_x, cnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "admm.in.xinit", x_init, cnt, flags, &xi));
    double *xo = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, cnt, flags, &xo));
    for (int b = 0; b < batch; ++b) {
        const size_t o = (size_t)b * P;
        const AdmmItem it{yd + o, off(md, o), off(td, o), off(xi, o), xo + o};
        SBTV_TRY(solve_with_exact_repeat(ctx, !(opts->speculate & 2), [&](bool spec) { return one(b, it, spec); }));
    }
    SBTV_TRY(stage_out_copy(ctx, x_out, xo, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_CSALSA_v2(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                   const double *mu1, const double *mu2, const double *sigma, const double *epsilon,
                   double continuationfactor, const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                   double *x_out, double *objective, double *distance1, double *distance2, double *criterion,
                   double *times, double *mses, int *numA, int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "CSALSA_v2", y, taps, opts, x_init, M, N, batch, taille));
    if (!mu1 || !mu2 || !sigma) return fail(ctx, SBTV_ERR_BADARG, "CSALSA_v2: missing required argument");
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0))
            return fail(ctx, SBTV_ERR_MISSING_LS, "(A^T A + mu I)^(-1) must be specified: mu1, mu2 must be > 0");
    const size_t t2 = (size_t)taille * taille;
    return admm_batch(
        ctx, M, N, batch, opts, y, nullptr, true_x, x_init, x_out, flags,
        [&](sbtv_group *lg) {
            return csalsa_sharded(lg, y, M, N, batch, taps, taille, mu1, mu2, sigma, epsilon, continuationfactor, opts, true_x,
                                  x_init, x_out, objective, distance1, distance2, criterion, times, mses, numA, numAt,
                                  n_outer, flags);
        },
        [&](int b, const AdmmItem &it, bool spec) {
            const size_t r = (size_t)b * opts->maxiter;                  // every trace row has maxiter entries
            return csalsa_one(ctx, it.y, M, N, taps + b * t2, taille, mu1[b], mu2[b], sigma[b], epsilon ? epsilon[b] : 0.0,
                              continuationfactor, opts, it.tru, it.x_init, it.x, off(objective, r), off(distance1, r),
                              off(distance2, r), off(criterion, r), off(times, r), off(mses, r), off(numA, b), off(numAt, b),
                              off(n_outer, b), spec);
        });
}

int sbtv_CoRAL_v2(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                  const double *tau1, const double *tau2, const double *mu1, const double *mu2, const double *mu_ls,
                  int TViters2, const sbtv_salsa_opts *opts, const double *true_x, const double *x_init, double *x_out,
                  double *objective, double *distance, double *times, double *mses, int *numA, int *numAt, int *n_outer,
                  int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "CoRAL_v2", y, taps, opts, x_init, M, N, batch, taille));
    if (!tau1 || !tau2 || !mu1 || !mu2) return fail(ctx, SBTV_ERR_BADARG, "CoRAL_v2: missing required argument");
    if (TViters2 <= 0) return fail(ctx, SBTV_ERR_MAXITER, "CoRAL_v2: TViters2 must be positive");
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0) || (mu_ls && !(mu_ls[b] > 0.0)))
            return fail(ctx, SBTV_ERR_MISSING_LS, "(A^T A + mu I)^(-1) must be specified: mu1, mu2 must be > 0");
    const size_t t2 = (size_t)taille * taille, mi = (size_t)opts->maxiter;
    return admm_batch(
        ctx, M, N, batch, opts, y, nullptr, true_x, x_init, x_out, flags,
        [&](sbtv_group *lg) {
            return coral_sharded(lg, y, M, N, batch, taps, taille, tau1, tau2, mu1, mu2, mu_ls, TViters2, opts, true_x, x_init,
                                 x_out, objective, distance, times, mses, numA, numAt, n_outer, flags);
        },
        [&](int b, const AdmmItem &it, bool spec) {
            return coral_one(ctx, it.y, M, N, taps + b * t2, taille, tau1[b], tau2[b], mu1[b], mu2[b],
                             mu_ls ? mu_ls[b] : mu1[b] + mu2[b], TViters2, opts, it.tru, it.x_init, it.x,
                             off(objective, b * (mi + 1)), off(distance, b * mi * 2), off(times, b * (mi + 1)),
                             off(mses, b * (mi + 1)), off(numA, b), off(numAt, b), off(n_outer, b), spec);
        });
}

int sbtv_SALSA_masked(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch, const double *taps,
                      int taille, const double *tau, const double *mu1, const double *mu2, const sbtv_salsa_opts *opts,
                      const double *true_x, const double *x_init, double *x_out, double *objective, double *distance,
                      double *times, double *mses, int *numA, int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "SALSA_masked", y, taps, opts, x_init, M, N, batch, taille));
    if (!mask) return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked: the mask is missing");
    if (!tau || !mu1 || !mu2) return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked: missing required argument");
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0)) return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked: mu1, mu2 must be > 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    const size_t P = (size_t)M * N, cnt = P * batch;
    if (!(flags & SBTV_DEVICE_PTRS))
        for (size_t i = 0; i < cnt; ++i)
            if (!(mask[i] >= 0.0) || std::isinf(mask[i]))
                return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked: the mask must be finite and non-negative");
    const size_t t2 = (size_t)taille * taille, mi = (size_t)opts->maxiter;
    return admm_batch(
        ctx, M, N, batch, opts, y, mask, true_x, x_init, x_out, flags,
        [&](sbtv_group *lg) {
            return masked_sharded(lg, y, mask, M, N, batch, taps, taille, tau, mu1, mu2, opts, true_x, x_init, x_out, objective,
                                  distance, times, mses, numA, numAt, n_outer, flags);
        },
        [&](int b, const AdmmItem &it, bool spec) {
            return masked_one(ctx, it.y, it.mask, M, N, taps + b * t2, taille, tau[b], mu1[b], mu2[b], opts, it.tru, it.x_init,
                              it.x, off(objective, b * (mi + 1)), off(distance, b * mi * 2), off(times, b * (mi + 1)),
                              off(mses, b * (mi + 1)), off(numA, b), off(numAt, b), off(n_outer, b), spec);
        });
}

}  // extern "C"

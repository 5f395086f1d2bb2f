// SK-ROCK chain on the TV posterior at FIXED parameters: the target, the closures and the Philox counters of
// sbtv_myula (sapg.hip), with the explicit stabilised step of Pereyra, Vargas Mieles, Zygalakis (SIAM J. Imaging Sci. 2020) in
// place of the Euler-Maruyama step.  include/sbtv.h states the algorithm; the coefficient table is sbtv_skrock_coefficients.
//
// One step is `stages` drift evaluations - a cold Chambolle prox (prox_iterate) and op_gradf on the stage's input, then one
// element-wise stage kernel - and one residual pass (op_resid) on the new sample.  Two image buffers alternate: stage j reads
// K_{j-1} (U) and K_{j-2} (V) and writes K_j over V; the last stage also writes the perturbed state P of the next step over
// U, so the new sample and P_next swap buffers when `stages` is odd.  Every stage kernel re-arms the prox control blocks for
// the cold prox that follows it (ProxArm), as myula_plain_kernel does.  The kernels and the host side of a step - stage table,
// noise feed, perturb launch, stage dispatch, buffer parity - are SkrockStepper of skrock_stage.inc, shared with sapg_skrock.hip;
// the moments request and the pooled check are mom_resolve / check_one_posterior (sampler_common.hip).
//
// Traces.  Ring slot r holds, for ONE sample ii, the accumulators of its residual pass and the partial sums of TVnorm(X(ii))
// (from the forward column pass of that residual pass where fft_cols_tv_ok allows, else from tvnorm_partials):
// skrock_trace_kernel turns up to SK_RING slots into gx / logpi in one launch, one workgroup per chain and slot, every sum in
// a fixed order.
//
// Moments.  X(ii) is accumulated in the registers of the last stage kernel; unselected samples launch the plain kernel.
#include <cmath>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

#include "skrock_stage.inc"      // SKB, SkrockStage, skrock_arm, skrock_perturb_kernel, skrock_stage_kernel
constexpr int SK_RING = 1024;     // samples between two trace launches (and two synchronisations)

struct SkrockDev {
    const double *theta, *sigma2; // [batch]
    const double *part;          // ring [slot][batch][ntv]: partial sums of TVnorm(X(ii))
    const double *acc;           // ring [slot][batch][3][nrb]: accumulators of the residual pass of X(ii), q = 0: ||A X - y||^2
    double *gx, *logpi;          // [batch][samples]
    int batch, ntv, nrb, samples;
    double parseval;
};

// gx(ii) and logpi(ii) of the samples ii0, ii0 + 1, ... in the ring slots 0, 1, ...: grid (batch, slots)
__global__ __launch_bounds__(SKB) void skrock_trace_kernel(SkrockDev u, int ii0) {
    __shared__ double red[4];
    const int b = blockIdx.x, s = blockIdx.y, ii = ii0 + s;
    const double *a = u.acc + ((size_t)s * u.batch + b) * 3 * u.nrb;
    const double *p = u.part + ((size_t)s * u.batch + b) * u.ntv;
    double r = 0.0, g = 0.0;
    for (int i = threadIdx.x; i < u.nrb; i += SKB) r += a[i];
    r = wav_block_sum(r, red);
    for (int i = threadIdx.x; i < u.ntv; i += SKB) g += p[i];
    g = wav_block_sum(g, red);
    const double f = (r * u.parseval) / (2 * u.sigma2[b]);
    if (threadIdx.x == 0) {
        u.gx[(size_t)b * u.samples + (ii - 1)] = g;
        u.logpi[(size_t)b * u.samples + (ii - 1)] = -f - u.theta[b] * g;
    }
}

inline bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_skrock(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                const sbtv_skrock_opts *op, const double *theta, const double *sigma2, const double *x0, const double *noise,
                double *gx, double *logpi, double *x_last, const sbtv_moments_opts *mo, double *post_mean, double *post_var,
                long long *post_count, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!y || !taps || !op || !theta || !sigma2 || batch < 1)
        return fail(ctx, SBTV_ERR_BADARG, "skrock: missing required argument (y, taps, op, theta, sigma2, batch >= 1)");
    if (op->samples < 2) return fail(ctx, SBTV_ERR_BADARG, "skrock: need samples >= 2");
    if (op->stages < 2) return fail(ctx, SBTV_ERR_BADARG, "skrock: need stages >= 2");
    if (!positive_finite(op->lambda) || !positive_finite(op->delta) || !positive_finite(op->eta))
        return fail(ctx, SBTV_ERR_BADARG, "skrock: lambda, delta and eta must be finite and > 0");
    for (int b = 0; b < batch; ++b)
        if (!positive_finite(theta[b]) || !positive_finite(sigma2[b]))
            return fail(ctx, SBTV_ERR_BADARG, "skrock: every theta[b] and sigma2[b] must be finite and > 0");
    if (op->chain_offset < 0) return fail(ctx, SBTV_ERR_BADARG, "skrock: chain_offset must be >= 0");
    if (op->chambolleit <= 0) return fail(ctx, SBTV_ERR_MAXITER, "skrock: chambolleit must be positive");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    SBTV_TRY(check_even_pixels(ctx, M, N));
    const int samples = op->samples, stages = op->stages, chambolleit = op->chambolleit;
    const size_t P = (size_t)M * N, cnt = P * batch, t2 = (size_t)taille * taille;
    const bool dev = (flags & SBTV_DEVICE_PTRS) != 0;
    // the moments request: the checks of sbtv_myula_moments
    MomReq sel{};
    const MomReq *selp = nullptr;
    SBTV_TRY(mom_resolve(ctx, "skrock", mo, 1, samples, post_mean, post_var, post_count, dev, &sel, &selp));
    if (selp && sel.pooled && batch > 1)
        SBTV_TRY(check_one_posterior(ctx, "skrock", y, P, taps, taille, theta, sigma2, batch, dev));
    const double lambda = op->lambda;

    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    BlurOp bop;
    SBTV_TRY(op_open(ctx, "skrock", M, N, batch, "Y", &bop));
    ProxPlan pp;
    SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
    const bool traces = gx || logpi, tv_fused = fft_cols_tv_ok(bop.fp), noise_host = noise && !dev;
    const int nrb = fft_rows_blocks(bop.fp);
    const int ring = samples < SK_RING ? samples : SK_RING;
    const double *yd = nullptr, *x0d = nullptr;
    SBTV_TRY(stage_in(ctx, "skrock.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "skrock.grad", x0, cnt, flags, &x0d));            // staged where the gradient goes later
    double *A = nullptr, *K = nullptr, *prox = nullptr, *grad = nullptr, *Z = nullptr, *par = nullptr, *acc_g = nullptr,
           *acc = nullptr, *part = nullptr, *tr_d = nullptr, *pm_mean = nullptr, *pm_m2 = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "skrock.X", x_last, cnt, flags, &A));
    SBTV_TRY(ws_get_t(ctx, "skrock.K", cnt, &K));                            // the second image buffer
    SBTV_TRY(ws_get_t(ctx, "skrock.prox", cnt, &prox));
    SBTV_TRY(ws_get_t(ctx, "skrock.grad", cnt, &grad));
    if (noise_host) SBTV_TRY(ws_get_t(ctx, "skrock.Z", cnt, &Z));
    const size_t accn = (size_t)batch * 3 * nrb;
    SBTV_TRY(ws_get_t(ctx, "skrock.accg", accn, &acc_g));                    // residual sums of the gradient passes: not used
    if (selp) {
        SBTV_TRY(ws_get_t(ctx, "skrock.pm_mean", cnt, &pm_mean));
        SBTV_TRY(ws_get_t(ctx, "skrock.pm_m2", cnt, &pm_m2));
    }
    const size_t npar = t2 * batch + 3 * (size_t)batch;
    SBTV_TRY(ws_get_t(ctx, "skrock.par", npar, &par));                       // [taps | lambda*theta | sigma2 | theta]
    double *taps_d = par, *lam_d = par + t2 * batch, *sig_d = lam_d + batch, *th_d = sig_d + batch;
    const size_t bs = (size_t)batch * samples, trlen = 2 * bs;
    {
        std::vector<double> hp(npar);
        for (size_t i = 0; i < t2 * batch; ++i) hp[i] = taps[i];
        for (int b = 0; b < batch; ++b) {
            hp[t2 * batch + b] = lambda * theta[b];                          // proxG(x, lambda, theta)   (run_deblur_tv.m:126)
            hp[t2 * batch + batch + b] = sigma2[b];
            hp[t2 * batch + 2 * (size_t)batch + b] = theta[b];
        }
        SBTV_HIP(ctx, hipMemcpyAsync(par, hp.data(), sizeof(double) * npar, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));                    // the staging vector goes out of scope
    }
    SBTV_TRY(psf_spectrum(ctx, bop.fp, taps_d, taille, bop.Hs));
    SBTV_TRY(op_spectrum(ctx, bop.fp, yd, nullptr, bop.S, bop.Ys));
    // X(1) = x0, or y
    const double *start = x0d ? x0d : yd;
    if (start != A) SBTV_HIP(ctx, hipMemcpyAsync(A, start, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, nullptr));
    const ProxArm arm{pp.ctrl, lam_d, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, nullptr};

    // the traces: TVnorm(X(ii)) partials and the residual accumulators of sample ii in ring slot `slot`
    SkrockDev u{};
    int ntv = tv_fused ? fft_cols_blocks(bop.fp) : 0;
    auto residual_pass = [&](const double *x, int slot) -> int {
        if (tv_fused) return op_resid(ctx, bop, x, acc + (size_t)slot * accn, nullptr, part + (size_t)slot * batch * ntv);
        double *tvp = nullptr;
        int n = 0;
        SBTV_TRY(tvnorm_partials(ctx, x, M, N, batch, &tvp, &n));            // arbitrary-size path
        if (!part) {                                                         // sample 1: the partial count is known now
            ntv = n;
            SBTV_TRY(ws_get_t(ctx, "skrock.part", (size_t)ring * batch * ntv, &part));
            u.part = part;
            u.ntv = ntv;
        }
        SBTV_HIP(ctx, hipMemcpyAsync(part + (size_t)slot * batch * ntv, tvp, sizeof(double) * batch * ntv,
                                     hipMemcpyDeviceToDevice, ctx->stream));
        return op_resid(ctx, bop, x, acc + (size_t)slot * accn);
    };
    auto trace = [&](int slots, int ii0) -> int {
        hipLaunchKernelGGL(skrock_trace_kernel, dim3(batch, slots), dim3(SKB), 0, ctx->stream, u, ii0);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };
    if (traces) {
        SBTV_TRY(ws_get_t(ctx, "skrock.acc", (size_t)ring * accn, &acc));
        if (tv_fused) SBTV_TRY(ws_get_t(ctx, "skrock.part", (size_t)ring * batch * ntv, &part));
        SBTV_TRY(ws_get_t(ctx, "skrock.traces", trlen, &tr_d));
        SBTV_HIP(ctx, hipMemsetAsync(tr_d, 0, sizeof(double) * trlen, ctx->stream));
        u.theta = th_d; u.sigma2 = sig_d; u.part = part; u.acc = acc; u.gx = tr_d; u.logpi = tr_d + bs; u.batch = batch;
        u.ntv = ntv; u.nrb = nrb; u.samples = samples; u.parseval = bop.parseval;
    }

    // the steps: the sample sits in sk.X, the caller's buffer or the second one, as the parity of the stage count has it
    SkrockStepper sk{ctx, &bop, &pp, arm, NoiseFeed{ctx, noise, Z, cnt}, A, K, prox, grad, acc_g, sig_d, pm_mean, pm_m2, lambda, P,
                     batch, stages, chambolleit, op->seed, (unsigned)op->chain_offset};
    SBTV_TRY(sk.table(op->eta, op->delta));

    // sample 1: the start state
    if (mom_sample_of(selp, 1)) SBTV_TRY(moments_seed(ctx, sk.X, pm_mean, pm_m2, P, batch));
    int filled = 0;                                                          // ring slots waiting for the trace kernel
    if (traces) {
        SBTV_TRY(residual_pass(sk.X, 0));
        filled = 1;
    }
    for (int ii = 2; ii <= samples; ++ii) {
        SBTV_TRY(sk.step(mom_sample_of(selp, ii), ii < samples));
        if (traces) {
            SBTV_TRY(residual_pass(sk.X, filled));
            if (++filled == ring || ii == samples) {
                SBTV_TRY(trace(filled, ii - filled + 1));
                if (filled == SK_RING) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
                filled = 0;
            }
        } else if ((ii - 1) % SK_RING == 0) {
            SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    }

    if (selp) SBTV_TRY(moments_finish(ctx, pm_mean, pm_m2, P, batch, mom_count(sel, samples), sel));
    std::vector<double> tr(traces ? trlen : 0);
    if (traces) SBTV_HIP(ctx, hipMemcpyAsync(tr.data(), tr_d, sizeof(double) * trlen, hipMemcpyDeviceToHost, ctx->stream));
    // the last sample sits in the caller's buffer or in the second one, as the parity of the stage count has it
    if (dev && x_last && sk.X != x_last)
        SBTV_HIP(ctx, hipMemcpyAsync(x_last, sk.X, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(stage_out_copy(ctx, x_last, sk.X, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < bs && traces; ++i) {
        if (gx) gx[i] = tr[i];
        if (logpi) logpi[i] = tr[bs + i];
    }
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

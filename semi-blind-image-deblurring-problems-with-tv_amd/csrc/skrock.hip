// SK-ROCK chain on the TV posterior at FIXED parameters: the target, the closures and the Philox counters of
// sbtv_myula (sapg.hip), with the explicit stabilised step of Pereyra, Vargas Mieles, Zygalakis (SIAM J. Imaging Sci. 2020) in
// place of the Euler-Maruyama step.  include/sbtv.h states the algorithm; the coefficient table is sbtv_skrock_coefficients.
//
// One step is `stages` drift evaluations - a cold Chambolle prox (prox_iterate) and op_gradf on the stage's input, then one
// element-wise stage kernel - and one residual pass (op_resid) on the new sample.  Two image buffers alternate: stage j reads
// K_{j-1} (U) and K_{j-2} (V) and writes K_j over V; the last stage also writes the perturbed state P of the next step over
// U, so the new sample and P_next swap buffers when `stages` is odd.  Every stage kernel re-arms the prox control blocks for
// the cold prox that follows it (ProxArm), as myula_plain_kernel does.
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
    if (mo) {
        if (!post_mean) return fail(ctx, SBTV_ERR_BADARG, "skrock: moments options and post_mean are required");
        const int first = mo->first == 0 ? 1 : mo->first;
        if (mo->thin < 1 || first < 1 || first > samples)
            return fail(ctx, SBTV_ERR_BADARG, "skrock: need thin >= 1 and 1 <= first <= samples");
        sel = MomReq{first, mo->thin, mo->pooled ? 1 : 0, post_mean, post_var, post_count, dev, false};
        selp = &sel;
        if (sel.pooled && batch > 1) {
            // pooling needs chains of ONE posterior: the same y, taps, theta and sigma2 in every chain
            bool same = true;
            for (int b = 1; same && b < batch; ++b)
                same = theta[b] == theta[0] && sigma2[b] == sigma2[0] && !memcmp(taps, taps + b * t2, sizeof(double) * t2);
            if (same) {
                std::vector<double> yh;
                const double *yv = y;
                if (dev) {
                    SBTV_HIP(ctx, hipSetDevice(ctx->device));
                    yh.resize(cnt);
                    SBTV_HIP(ctx, hipMemcpy(yh.data(), y, sizeof(double) * cnt, hipMemcpyDeviceToHost));
                    yv = yh.data();
                }
                for (int b = 1; same && b < batch; ++b) same = !memcmp(yv, yv + b * P, sizeof(double) * P);
            }
            if (!same) return fail(ctx, SBTV_ERR_BADARG, "skrock: pooled = 1 needs chains with the same y, taps, theta and sigma2");
        }
    } else if (post_mean || post_var || post_count) {
        return fail(ctx, SBTV_ERR_BADARG, "skrock: moment outputs without moments options");
    }

    // the coefficient table and the scalars of the stages
    std::vector<double> mu(stages), nu(stages), kappa(stages);
    SBTV_TRY(sbtv_skrock_coefficients(stages, op->eta, mu.data(), nu.data(), kappa.data(), nullptr, nullptr));
    const double lambda = op->lambda, delta = op->delta, q = sqrt(2 * delta), nu1q = nu[0] * q;
    std::vector<SkrockStage> st(stages);
    st[0] = SkrockStage{mu[0] * delta, 0.0, kappa[0] * q, nu1q};
    for (int j = 1; j < stages; ++j) st[j] = SkrockStage{mu[j] * delta, nu[j], kappa[j], nu1q};

    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    BlurOp bop;
    SBTV_TRY(op_open(ctx, "skrock", M, N, batch, "Y", &bop));
    ProxPlan pp;
    SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
    const bool traces = gx || logpi, tv_fused = fft_cols_tv_ok(bop.fp), noise_host = noise && !dev;
    const int nrb = fft_rows_blocks(bop.fp), nblk = ew_blocks(P);
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

    // the normals of `step` as the kernels read them: the staging buffer, the caller's device array, or null: Philox
    auto stage_noise = [&](unsigned step) -> int {
        if (!noise_host) return 0;
        SBTV_HIP(ctx, hipMemcpyAsync(Z, noise + (size_t)step * cnt, sizeof(double) * cnt, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    };
    auto normals = [&](unsigned step) -> const double * {
        if (noise_host) return Z;
        return noise ? noise + (size_t)step * cnt : nullptr;
    };
    const dim3 grid(nblk, batch), block(SKB);
    // one stage: the drift at U (prox and gradient), then the stage kernel
    auto stage = [&](double *U, double *V, int j, bool next_p, const RngArgs &r, const MomArgs *mc) -> int {
        const bool first = j == 1, last = j == stages, np = last && next_p, mo_on = last && mc && mc->k > 0;
        SBTV_TRY(prox_iterate(ctx, pp, U, chambolleit, prox, true));
        SBTV_TRY(op_gradf(ctx, bop, U, acc_g, grad));
        const double *zd = first ? normals(r.step) : (np ? normals(r.step + 1u) : nullptr);
        const SkrockStage &sj = st[j - 1];
#define SBTV_SKROCK_STAGE(F, L, NX, MO, momarg)                                                                           \
    hipLaunchKernelGGL((skrock_stage_kernel<F, L, NX, MO>), grid, block, 0, ctx->stream, U, V, (const double *)prox,         \
                       (const double *)grad, zd, (const double *)sig_d, lambda, sj, P, r, arm, momarg)
        if (first)
            SBTV_SKROCK_STAGE(true, false, false, false, SkNoMom{});
        else if (!last)
            SBTV_SKROCK_STAGE(false, false, false, false, SkNoMom{});
        else if (np && mo_on)
            SBTV_SKROCK_STAGE(false, true, true, true, *mc);
        else if (np)
            SBTV_SKROCK_STAGE(false, true, true, false, SkNoMom{});
        else if (mo_on)
            SBTV_SKROCK_STAGE(false, true, false, true, *mc);
        else
            SBTV_SKROCK_STAGE(false, true, false, false, SkNoMom{});
#undef SBTV_SKROCK_STAGE
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };

    double *X = A, *Pb = K;                                                  // the sample; the perturbed state of the next step
    // sample 1: the start state
    if (mom_sample_of(selp, 1)) SBTV_TRY(moments_seed(ctx, X, pm_mean, pm_m2, P, batch));
    int filled = 0;                                                          // ring slots waiting for the trace kernel
    if (traces) {
        SBTV_TRY(residual_pass(X, 0));
        filled = 1;
    }
    for (int ii = 2; ii <= samples; ++ii) {
        const RngArgs r{op->seed, (unsigned)(ii - 2), (unsigned)op->chain_offset, nullptr};
        const bool more = ii < samples;
        if (ii == 2) {
            SBTV_TRY(stage_noise(r.step));
            hipLaunchKernelGGL(skrock_perturb_kernel, grid, block, 0, ctx->stream, (const double *)X, Pb, normals(r.step), nu1q,
                               P, r, arm);
            SBTV_HIP(ctx, hipGetLastError());
        }
        double *U = Pb, *V = X;                                              // K_{j-1} (stage 1: P), K_{j-2}
        SBTV_TRY(stage(U, V, 1, false, r, nullptr));
        if (more) SBTV_TRY(stage_noise(r.step + 1u));                        // after FIRST, before LAST
        for (int j = 2; j <= stages; ++j) {
            const MomArgs mc{pm_mean, pm_m2, j == stages ? mom_sample_of(selp, ii) : 0, nullptr, 1, 1};
            SBTV_TRY(stage(U, V, j, more, r, &mc));
            std::swap(U, V);                                                 // U = K_j, V = K_{j-1} (after the last: P_next)
        }
        X = U;
        Pb = V;
        if (traces) {
            SBTV_TRY(residual_pass(X, filled));
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
    if (dev && x_last && X != x_last)
        SBTV_HIP(ctx, hipMemcpyAsync(x_last, X, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(stage_out_copy(ctx, x_last, X, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < bs && traces; ++i) {
        if (gx) gx[i] = tr[i];
        if (logpi) logpi[i] = tr[bs + i];
    }
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

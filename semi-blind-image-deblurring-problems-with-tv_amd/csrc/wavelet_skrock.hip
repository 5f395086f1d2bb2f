// SK-ROCK chain on the coefficients of the redundant wavelet frame at a FIXED theta: the target, the
// operators, the traces and the moments of sbtv_myula_wavelet (wavelet_myula.hip), with the explicit stabilised step of
// Pereyra, Vargas Mieles, Zygalakis (SIAM J. Imaging Sci. 2020) in place of the Euler-Maruyama step.  include/sbtv.h states
// the algorithm.
//
// One step is `stages` gradient passes (wav_chain_spectrum + wav_chain_rows(OP_GRADF) on a copy of the WavChain whose X is
// the stage's input), each followed by one element-wise stage kernel (wavelet_chain.hip), and one residual pass (OP_RESID)
// on the new sample.  Two coefficient buffers alternate: stage j writes K_j over K_{j-2}; the last stage also writes the
// perturbed state P of the next step over K_{s-1}, so the new sample and P_next swap buffers when `stages` is odd.
//
// Traces.  Ring slot r holds, for ONE sample ii, the accumulators of its residual pass and the partial sums of |X(ii)| (the
// last stage kernel; wav_abs_sum for the start state): wav_skrock_trace_kernel turns up to WS_RING slots into gx / logpi in
// one launch, one workgroup per chain and slot, every sum in a fixed order.
//
// Moments.  The image W X(ii) is accumulated inside the level-1 synthesis of the residual pass of sample ii, the
// coefficients X(ii) in the registers of the last stage kernel.  Unselected samples launch the plain kernels.
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

constexpr int WS_RING = 1024;     // samples between two trace launches (and two synchronisations)

struct WavSkrockDev {
    const double *par;           // [2][batch]: theta | sigma2
    const double *part;          // ring [slot][batch][nblk]: partial sums of |X(ii)|
    const double *acc;           // ring [slot][batch][3][nrb]: accumulators of the residual pass of X(ii), q = 0: ||B W X - y||^2
    double *gx, *logpi;          // [batch][samples]
    int batch, nblk, nrb, samples;
    double parseval;
};

// gx(ii) and logpi(ii) of the samples ii0, ii0 + 1, ... in the ring slots 0, 1, ...: grid (batch, slots)
__global__ __launch_bounds__(WAV_EWB) void wav_skrock_trace_kernel(WavSkrockDev u, int ii0) {
    __shared__ double red[4];
    const int b = blockIdx.x, s = blockIdx.y, ii = ii0 + s;
    const double *a = u.acc + ((size_t)s * u.batch + b) * 3 * u.nrb;
    const double *p = u.part + ((size_t)s * u.batch + b) * u.nblk;
    double r = 0.0, g = 0.0;
    for (int i = threadIdx.x; i < u.nrb; i += WAV_EWB) r += a[i];
    r = wav_block_sum(r, red);
    for (int i = threadIdx.x; i < u.nblk; i += WAV_EWB) g += p[i];
    g = wav_block_sum(g, red);
    const double f = (r * u.parseval) / (2 * u.par[u.batch + b]);
    if (threadIdx.x == 0) {
        u.gx[(size_t)b * u.samples + (ii - 1)] = g;
        u.logpi[(size_t)b * u.samples + (ii - 1)] = -f - u.par[b] * g;
    }
}

inline bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

// the table of include/sbtv.h (sbtv_skrock_coefficients): mu, nu, kappa [stages] (entry j - 1 is stage j)
void skrock_table(int s, double eta, double *mu, double *nu, double *kappa, double *omega, double *ls) {
    const double w0 = 1.0 + eta / ((double)s * (double)s);
    std::vector<double> T(s + 1), U(s + 1);
    T[0] = 1.0;
    T[1] = w0;
    U[0] = 1.0;
    U[1] = 2.0 * w0;
    for (int j = 2; j <= s; ++j) {
        T[j] = 2.0 * w0 * T[j - 1] - T[j - 2];
        U[j] = 2.0 * w0 * U[j - 1] - U[j - 2];
    }
    const double w1 = T[s] / ((double)s * U[s - 1]);
    if (mu) mu[0] = w1 / w0;
    if (nu) nu[0] = (double)s * w1 / 2.0;
    if (kappa) kappa[0] = (double)s * w1 / w0;
    for (int j = 2; j <= s; ++j) {
        const double nj = 2.0 * w0 * T[j - 1] / T[j];
        if (mu) mu[j - 1] = 2.0 * w1 * T[j - 1] / T[j];
        if (nu) nu[j - 1] = nj;
        if (kappa) kappa[j - 1] = 1.0 - nj;
    }
    if (omega) {
        omega[0] = w0;
        omega[1] = w1;
    }
    if (ls) *ls = ((double)s - 0.5) * ((double)s - 0.5) * (2.0 - 4.0 * eta / 3.0) - 1.5;
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_skrock_coefficients(int stages, double eta, double *mu, double *nu, double *kappa, double *omega, double *ls) {
    if (stages < 2 || !positive_finite(eta))
        return fail(nullptr, SBTV_ERR_BADARG, "sbtv_skrock_coefficients: need stages >= 2 and a finite eta > 0");
    skrock_table(stages, eta, mu, nu, kappa, omega, ls);
    return 0;
}

int sbtv_skrock_max_step(int stages, double eta, double sigma2, double lambda, double normB2, double *delta_max) {
    if (stages < 2 || !positive_finite(eta) || !positive_finite(sigma2) || !positive_finite(lambda) || !(normB2 >= 0.0) ||
        !std::isfinite(normB2) || !delta_max)
        return fail(nullptr, SBTV_ERR_BADARG,
                    "sbtv_skrock_max_step: need stages >= 2, finite eta, sigma2, lambda > 0, a finite normB2 >= 0 and delta_max");
    double ls = 0.0;
    skrock_table(stages, eta, nullptr, nullptr, nullptr, nullptr, &ls);
    *delta_max = ls / (normB2 / sigma2 + 1.0 / lambda);
    return 0;
}

int sbtv_skrock_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                        const double *h, int hlen, int levels, const sbtv_skrock_wavelet_opts *op, const double *theta,
                        const double *sigma2, const double *xw0, const double *noise, double *gx, double *logpi,
                        double *xw_last, const sbtv_moments_opts *mo, double *post_mean, double *post_var,
                        long long *post_count, double *coef_mean, double *coef_var, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!y || !op || !theta || !sigma2 || batch < 1)
        return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: missing required argument (y, op, theta, sigma2, batch >= 1)");
    if (!taps) return fail(ctx, SBTV_ERR_MISSING_AT, "The function handle for transpose of A is missing");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    if (op->samples < 2) return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: need samples >= 2");
    if (op->stages < 2) return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: need stages >= 2");
    if (!positive_finite(op->lambda) || !positive_finite(op->delta) || !positive_finite(op->eta))
        return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: lambda, delta and eta must be finite and > 0");
    for (int b = 0; b < batch; ++b)
        if (!positive_finite(theta[b]) || !positive_finite(sigma2[b]))
            return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: every theta[b] and sigma2[b] must be finite and > 0");
    if (op->chain_offset < 0) return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: chain_offset must be >= 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    const int samples = op->samples, stages = op->stages;
    const size_t P = (size_t)M * N, cnt = P * batch, dimX = P * wp.bands(), ccnt = dimX * batch;
    const bool dev = (flags & SBTV_DEVICE_PTRS) != 0;
    // the moments request: one selection for both domains
    MomReq sel{};
    const MomReq *selp = nullptr;
    if (mo) {
        if (!post_mean && !coef_mean)
            return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: moments need post_mean or coef_mean");
        if ((post_var && !post_mean) || (coef_var && !coef_mean))
            return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: post_var needs post_mean and coef_var needs coef_mean");
    } else if (post_mean || post_var || post_count || coef_mean || coef_var) {
        return fail(ctx, SBTV_ERR_BADARG, "skrock_wavelet: moment outputs without moments options");
    }
    // MomReq's outputs are set per domain where the moments are finished
    SBTV_TRY(mom_resolve(ctx, "skrock_wavelet", mo, 1, samples, post_mean ? post_mean : coef_mean, nullptr, nullptr, dev, &sel, &selp));
    if (selp && sel.pooled && batch > 1)
        SBTV_TRY(check_one_posterior(ctx, "skrock_wavelet", y, P, taps, taille, theta, sigma2, batch, dev));
    const bool mom_img = selp && post_mean, mom_coef = selp && coef_mean;

    // the coefficient table and the scalars of the stages
    std::vector<double> mu(stages), nu(stages), kappa(stages);
    skrock_table(stages, op->eta, mu.data(), nu.data(), kappa.data(), nullptr, nullptr);
    const double delta = op->delta, q = sqrt(2 * delta), nu1q = nu[0] * q;
    std::vector<WavSkrockStage> st(stages);
    st[0] = WavSkrockStage{mu[0] * delta, 0.0, kappa[0] * q, nu1q};
    for (int j = 1; j < stages; ++j) st[j] = WavSkrockStage{mu[j] * delta, nu[j], kappa[j], nu1q};

    WavChain wc;
    SBTV_TRY(wav_chain_buffers(ctx, "wsk", wp, batch, y, xw0, noise, xw_last, flags, &wc));
    const int nblk = wc.nblk, nrb = wc.nrb;
    const int ring = samples < WS_RING ? samples : WS_RING;
    const size_t accn = (size_t)batch * 3 * nrb;
    double *K = nullptr, *par = nullptr, *taps_d = nullptr, *acc = nullptr, *acc_g = nullptr, *part = nullptr, *tr_d = nullptr,
           *im_mean = nullptr, *im_m2 = nullptr, *c_mean = nullptr, *c_m2 = nullptr;
    SBTV_TRY(ws_get_t(ctx, "wsk.K", ccnt, &K));                              // the second coefficient buffer
    SBTV_TRY(ws_get_t(ctx, "wsk.acc", (size_t)ring * accn, &acc));
    SBTV_TRY(ws_get_t(ctx, "wsk.accg", accn, &acc_g));                       // Parseval sums of the gradient passes: not used
    SBTV_TRY(ws_get_t(ctx, "wsk.part", (size_t)ring * batch * nblk, &part));
    const size_t t2b = (size_t)taille * taille * batch, npar = 2 * (size_t)batch + t2b;
    SBTV_TRY(ws_get_t(ctx, "wsk.par", npar, &par));                          // [theta | sigma2 | taps]
    taps_d = par + 2 * (size_t)batch;
    const size_t bs = (size_t)batch * samples, trlen = 2 * bs;
    SBTV_TRY(ws_get_t(ctx, "wsk.traces", trlen, &tr_d));
    if (mom_img) {
        SBTV_TRY(ws_get_t(ctx, "wsk.im_mean", cnt, &im_mean));
        SBTV_TRY(ws_get_t(ctx, "wsk.im_m2", cnt, &im_m2));
    }
    if (mom_coef) {
        SBTV_TRY(ws_get_t(ctx, "wsk.c_mean", ccnt, &c_mean));
        SBTV_TRY(ws_get_t(ctx, "wsk.c_m2", ccnt, &c_m2));
    }
    WavSkrockDev u{};
    u.par = par; u.part = part; u.acc = acc; u.gx = tr_d; u.logpi = tr_d + bs; u.batch = batch; u.nblk = nblk; u.nrb = nrb;
    u.samples = samples; u.parseval = 1.0 / ((double)M * N);

    // constants, spectra of the PSF and of y, the start state
    {
        std::vector<double> hp(npar);
        for (int b = 0; b < batch; ++b) {
            hp[b] = theta[b];
            hp[batch + b] = sigma2[b];
        }
        for (size_t i = 0; i < t2b; ++i) hp[2 * (size_t)batch + i] = taps[i];
        SBTV_HIP(ctx, hipMemcpyAsync(par, hp.data(), sizeof(double) * npar, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(tr_d, 0, sizeof(double) * trlen, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));                    // the staging vector goes out of scope
    }
    SBTV_TRY(psf_spectrum(ctx, wc.op.fp, taps_d, taille, wc.op.Hs));
    SBTV_TRY(wav_chain_start(ctx, wc));

    const WavStepPar sp{par, par + batch, 1};
    // G = W' B'(B W K - y) of the coefficients in buffer `in` (the Parseval sum of the pass is not used)
    auto gradient_pass = [&](double *in) -> int {
        WavChain at = wc;
        at.X = in;
        SBTV_TRY(wav_chain_spectrum(ctx, at, nullptr));
        return wav_chain_rows(ctx, at, OP_GRADF, acc_g);
    };
    // ||B W X(ii) - y||^2 of the sample in buffer `in` -> the slot's accumulators; its image is accumulated while the
    // level-1 synthesis stores it
    auto residual_pass = [&](double *in, int slot, int ii) -> int {
        WavChain at = wc;
        at.X = in;
        const MomArgs ma{im_mean, im_m2, mom_img ? mom_sample_of(selp, ii) : 0, nullptr, 1, 1};
        SBTV_TRY(wav_chain_spectrum(ctx, at, &ma));
        return wav_chain_rows(ctx, at, OP_RESID, acc + (size_t)slot * accn);
    };
    // the traces of `slots` ring slots, the first of them sample ii0
    auto trace = [&](int slots, int ii0) -> int {
        hipLaunchKernelGGL(wav_skrock_trace_kernel, dim3(batch, slots), dim3(WAV_EWB), 0, ctx->stream, u, ii0);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };

    double *X = wc.X, *Pb = K;                                               // the sample; the perturbed state of the next step
    // sample 1: the start state
    SBTV_TRY(wav_abs_sum(ctx, wc, part));
    if (mom_coef && mom_sample_of(selp, 1)) SBTV_TRY(moments_seed(ctx, X, c_mean, c_m2, dimX, batch));
    SBTV_TRY(residual_pass(X, 0, 1));
    ctx->calls += batch;
    int filled = 1;                                                          // ring slots waiting for the trace kernel
    for (int ii = 2; ii <= samples; ++ii) {
        const RngArgs r{op->seed, (unsigned)(ii - 2), (unsigned)op->chain_offset, nullptr};
        const bool more = ii < samples;
        if (ii == 2) {
            SBTV_TRY(wav_skrock_noise(ctx, wc, r.step));
            SBTV_TRY(wav_skrock_perturb(ctx, wc, X, Pb, nu1q, r));
        }
        const int slot = filled;
        double *U = Pb, *V = X;                                              // K_{j-1} (stage 1: P), K_{j-2}
        SBTV_TRY(gradient_pass(U));
        SBTV_TRY(wav_skrock_stage(ctx, wc, sp, op->lambda, U, V, st[0], true, false, false, r, nullptr));
        if (more) SBTV_TRY(wav_skrock_noise(ctx, wc, r.step + 1u));          // after FIRST, before LAST
        for (int j = 2; j <= stages; ++j) {
            const bool last = j == stages;
            const MomArgs mc{c_mean, c_m2, last && mom_coef ? mom_sample_of(selp, ii) : 0, nullptr, 1, 1};
            SBTV_TRY(gradient_pass(U));
            SBTV_TRY(wav_skrock_stage(ctx, wc, sp, op->lambda, U, V, st[j - 1], false, last, more, r,
                                      part + (size_t)slot * batch * nblk, &mc));
            std::swap(U, V);                                                 // U = K_j, V = K_{j-1} (after the last: P_next)
        }
        X = U;
        Pb = V;
        SBTV_TRY(residual_pass(X, slot, ii));
        ctx->calls += (2 * (long long)stages + 1) * batch;
        if (++filled == ring || ii == samples) {
            SBTV_TRY(trace(filled, ii - filled + 1));
            if (filled == WS_RING) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            filled = 0;
        }
    }

    if (selp) {
        const long long n = mom_count(sel, samples);
        if (mom_img) {
            MomReq rq = sel;
            rq.mean = post_mean;
            rq.var = post_var;
            SBTV_TRY(moments_finish(ctx, im_mean, im_m2, P, batch, n, rq));
        }
        if (mom_coef) {
            MomReq rq = sel;
            rq.mean = coef_mean;
            rq.var = coef_var;
            SBTV_TRY(moments_finish(ctx, c_mean, c_m2, dimX, batch, n, rq));
        }
        for (int c = 0; post_count && c < (sel.pooled ? 1 : batch); ++c) post_count[c] = sel.pooled ? n * batch : n;
    }
    std::vector<double> tr(trlen);
    SBTV_HIP(ctx, hipMemcpyAsync(tr.data(), tr_d, sizeof(double) * trlen, hipMemcpyDeviceToHost, ctx->stream));
    // the last sample sits in the caller's buffer or in the second one, as the parity of the stage count has it
    if (dev && xw_last && X != xw_last)
        SBTV_HIP(ctx, hipMemcpyAsync(xw_last, X, sizeof(double) * ccnt, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(stage_out_copy(ctx, xw_last, X, ccnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < bs; ++i) {
        if (gx) gx[i] = tr[i];
        if (logpi) logpi[i] = tr[bs + i];
    }
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

// Empirical-Bayes estimate of the regularisation parameter theta of the wavelet-l1 prior: the MYULA chain
// on the coefficients of the redundant wavelet frame and the log-scale stochastic update of SALSA/SAPG_algorithm_1.m:120-216,
// as SALSA/run_deblur_synthesis_L1.m:125-156 sets them up (proxG = soft, g = l1, gradF = W' B'(B W xw - y) / sigma2).  Only the
// theta part of SAPG_algorithm_1.m is built: its second parameter `tau` needs op.to_init, op.grad_t and a two-argument gradF
// that the script never defines; csrc/wavelet_sapg_sb.hip builds that part with the PSF parameters as tau.
//
// The loop is device-resident.  The array-sized state is the chain X [batch][3J+1][M N] and the gradient; the prox is never
// stored: wav_step_kernel (wavelet_chain.hip, which holds what the three chain drivers share) recomputes soft(X, lambda theta)
// from X and the theta the reference formed it with, which lags one iteration.  One iteration: J synthesis launches, the FFT
// triple with OP_GRADF (whose Parseval sum is ||B W X - y||^2 of the state BEFORE the step), J analysis launches,
// wav_step_kernel (the whole element-wise update and the partial sums of |X_new|) and wav_sapg_update_kernel (one workgroup per chain: the sums in a fixed order, eta / theta, the traces).  The
// residual of sample ii is the one the next iteration computes anyway, so logpi(ii) is completed one iteration late; the last
// sample costs one extra synthesis + forward transform + OP_RESID.
#include <cmath>
#include <vector>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

// what the update kernel keeps per chain between two iterations
struct WavSapgChain {
    double eta;        // eta(ii-1)
    double th_prev;    // theta(ii-2): the theta the prox of the next MYULA step is formed with (theta(1) at ii = 2)
    double th_cur;     // theta(ii-1)
    double g_last;     // ||X||_1 of the current sample
    double sum_eta;    // sum of eta(burnIn .. ii-1)
    double n_eta;      // its number of terms
    double theta_eb;   // set by the last phase
    double sig2;       // sigma2, constant here: the step kernel reads it next to th_prev
};

// traces of all chains on the device: [batch][samples] each, wu [batch][wstride]
struct WavSapgTraces {
    double *thetas, *gx, *logpi, *mean, *tol, *wu;
};

struct WavSapgDev {
    WavSapgChain *chain;         // [batch]
    const double *part;          // [batch][nblk] partial sums of |X_new| (wav_chain_step / wav_abs_sum)
    const double *acc;           // [batch][3][nrb] accumulators of the row pass, q = 0: ||B W X - y||^2 (unscaled)
    int nblk, nrb, samples, warmup, wstride, burnIn;
    double parseval, dimX, min_eta, max_eta;
    WavSapgTraces tr;
};

enum { WS_PH_START = 0, WS_PH_WARMUP = 1, WS_PH_MAIN = 2, WS_PH_LAST = 3 };

// End of an iteration, one workgroup per chain.  R = ||B W X - y||^2 of the state before this iteration's step (the row
// pass), g = ||X_new||_1 (the step's partials), both summed in a fixed order.
//   WS_PH_START: no step yet, only g of the start state is booked (the partials of wav_abs_sum)
//   every other phase: the log-density of the PREVIOUS sample is completed with R (SAPG_algorithm_1.m:136,166,190)
//   WS_PH_MAIN, iteration ii: eta / theta (:180-182), gx (:191), tol_thetas / mean_thetas (:199-211)
//   WS_PH_LAST: nothing was stepped; R belongs to sample `samples`; theta_EB (:226)
__global__ __launch_bounds__(WAV_EWB) void wav_sapg_update_kernel(WavSapgDev u, int phase, int ii, double delta) {
    __shared__ double red[4];
    const int b = blockIdx.x, S = u.samples;
    double r = 0.0, g = 0.0;
    if (phase != WS_PH_START) {
        for (int i = threadIdx.x; i < u.nrb; i += WAV_EWB) r += u.acc[(size_t)b * 3 * u.nrb + i];
        r = wav_block_sum(r, red);
    }
    if (phase != WS_PH_LAST) {
        for (int i = threadIdx.x; i < u.nblk; i += WAV_EWB) g += u.part[(size_t)b * u.nblk + i];
        g = wav_block_sum(g, red);
    }
    if (threadIdx.x != 0) return;
    WavSapgChain c = u.chain[b];
    const double f = (r * u.parseval) / (2 * c.sig2);
    const double lp = -f - c.th_prev * c.g_last;            // logPi(previous sample, the theta it was stepped under)
    if (phase == WS_PH_START || phase == WS_PH_WARMUP) {
        if (phase == WS_PH_WARMUP && ii > 2) u.tr.wu[(size_t)b * u.wstride + (ii - 2)] = lp;              // logPiTrace_WU(ii-1)  (:136)
        c.g_last = g;
        u.chain[b] = c;
        return;
    }
    if (phase == WS_PH_LAST) {
        u.tr.logpi[(size_t)b * S + (S - 1)] = lp;                                // logPiTraceX(samples)  (:190)
        c.theta_eb = exp(c.sum_eta / c.n_eta);                                   // :226
        u.chain[b] = c;
        return;
    }
    if (ii == 2 && u.warmup >= 2) u.tr.wu[(size_t)b * u.wstride + (u.warmup - 1)] = lp;   // the last warm-up sample
    u.tr.logpi[(size_t)b * S + (ii - 2)] = lp;                                   // :166 (ii = 2), :190
    const WavThetaStep t = wav_theta_step(c.eta, c.th_cur, g, delta, u.dimX, u.min_eta, u.max_eta, ii >= u.burnIn, c.sum_eta,
                                          c.n_eta);                              // :180-182,199-211
    u.tr.thetas[(size_t)b * S + (ii - 1)] = t.th;
    u.tr.gx[(size_t)b * S + (ii - 2)] = g;                                       // :191
    u.tr.tol[(size_t)b * S + (ii - 1)] = t.tol;
    if (ii > u.burnIn) u.tr.mean[(size_t)b * S + (ii - u.burnIn - 1)] = t.mean;
    c.eta = t.eta;
    c.sum_eta = t.sum_eta;
    c.n_eta = t.n_eta;
    c.th_prev = c.th_cur;
    c.th_cur = t.th;
    c.g_last = g;
    u.chain[b] = c;
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_SAPG_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                      const double *h, int hlen, int levels, const sbtv_sapg_wavelet_opts *op, const double *xw0,
                      const double *noise, double *thetas, double *gx, double *logpi, double *logpi_wu, double *mean_thetas,
                      double *tol_thetas, double *theta_eb, double *xw_last, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!y || !op || !theta_eb || batch < 1) return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: missing required argument");
    if (!taps) return fail(ctx, SBTV_ERR_MISSING_AT, "The function handle for transpose of A is missing");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    if (op->samples < 2 || op->warmup < 0 || op->burnIn < 1 || op->burnIn > op->samples)
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: need samples >= 2, warmup >= 0, 1 <= burnIn <= samples");
    if (!(op->lambda > 0.0) || !(op->gamma > 0.0) || !(op->sigma2 > 0.0))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: lambda, gamma and sigma2 must be > 0");
    if (!(op->min_th > 0.0) || !(op->min_th <= op->th_init) || !(op->th_init <= op->max_th))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: need 0 < min_th <= th_init <= max_th");
    if (op->chain_offset < 0) return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: chain_offset must be >= 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    WavChain wc;
    SBTV_TRY(wav_chain_buffers(ctx, "wsapg", wp, batch, y, xw0, noise, xw_last, flags, &wc));
    const int samples = op->samples, warmup = op->warmup, wsteps = warmup > 0 ? warmup - 1 : 0, wstride = warmup > 0 ? warmup : 1;
    const size_t dimX = wc.dimX, ccnt = wc.ccnt;
    double *X = wc.X, *taps_d = nullptr, *acc = nullptr, *part = nullptr, *tr_d = nullptr;
    WavSapgDev u{};
    SBTV_TRY(ws_get_t(ctx, "wsapg.acc", (size_t)batch * 3 * wc.nrb, &acc));
    SBTV_TRY(ws_get_t(ctx, "wsapg.part", (size_t)batch * wc.nblk, &part));
    SBTV_TRY(ws_get_t(ctx, "wsapg.taps", (size_t)taille * taille * batch, &taps_d));
    SBTV_TRY(ws_get_t(ctx, "wsapg.chain", (size_t)batch, &u.chain));
    const size_t bs = (size_t)batch * samples, trlen = 5 * bs + (size_t)batch * wstride;
    SBTV_TRY(ws_get_t(ctx, "wsapg.traces", trlen, &tr_d));
    u.tr = WavSapgTraces{tr_d, tr_d + bs, tr_d + 2 * bs, tr_d + 3 * bs, tr_d + 4 * bs, tr_d + 5 * bs};
    u.part = part; u.acc = acc; u.nblk = wc.nblk; u.nrb = wc.nrb; u.samples = samples; u.warmup = warmup; u.wstride = wstride;
    u.burnIn = op->burnIn; u.parseval = 1.0 / ((double)M * N); u.dimX = (double)dimX;
    u.min_eta = log(op->min_th); u.max_eta = log(op->max_th);

    // constants, spectra of the PSF and of y, the start state
    const double eta_init = log(op->th_init);                                // :101
    {
        const WavSapgChain c0{eta_init, op->th_init, op->th_init, 0.0, op->burnIn == 1 ? eta_init : 0.0,
                              op->burnIn == 1 ? 1.0 : 0.0, 0.0, op->sigma2};
        std::vector<WavSapgChain> ch((size_t)batch, c0);
        SBTV_HIP(ctx, hipMemcpyAsync(u.chain, ch.data(), sizeof(WavSapgChain) * batch, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(taps_d, taps, sizeof(double) * taille * taille * batch, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(tr_d, 0, sizeof(double) * trlen, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));                    // the staging vector goes out of scope
    }
    SBTV_TRY(psf_spectrum(ctx, wc.op.fp, taps_d, taille, wc.op.Hs));
    SBTV_TRY(wav_chain_start(ctx, wc));
    auto update = [&](int phase, int ii, double delta) -> int {
        hipLaunchKernelGGL(wav_sapg_update_kernel, dim3(batch), dim3(WAV_EWB), 0, ctx->stream, u, phase, ii, delta);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };
    if (wsteps == 0) {
        // logPiTraceX(1) needs g of the start state (:166); after a warm-up the last warm-up step has left it
        SBTV_TRY(wav_abs_sum(ctx, wc, part));
        SBTV_TRY(update(WS_PH_START, 1, 0.0));
    }
    // the lagging theta and sigma2 of chain b, where the update kernel keeps them
    const WavStepPar sp{&u.chain->th_prev, &u.chain->sig2, (int)(sizeof(WavSapgChain) / sizeof(double))};
    // MYULA step number `step` of the call (warm-up steps first, as the noise array is laid out) and its update
    auto iteration = [&](size_t step, int phase, int ii) -> int {
        SBTV_TRY(wav_chain_spectrum(ctx, wc));
        SBTV_TRY(wav_chain_rows(ctx, wc, OP_GRADF, acc));                    // W' B'(B W X - y) -> G, ||B W X - y||^2 -> acc
        const RngArgs r{op->seed, (unsigned)step, (unsigned)op->chain_offset, nullptr};
        SBTV_TRY(wav_chain_step(ctx, wc, sp, op->gamma, op->lambda, r, part));
        // delta(ii) of :111
        SBTV_TRY(update(phase, ii, phase == WS_PH_MAIN ? op->d_scale * (pow((double)ii, -op->d_exp) / (double)dimX) : 0.0));
        ctx->calls += 2 * (long long)batch;
        return 0;
    };
    for (int ii = 2; ii <= warmup; ++ii) {                                   // :131-141
        SBTV_TRY(iteration((size_t)(ii - 2), WS_PH_WARMUP, ii));
        if ((ii & 1023) == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int ii = 2; ii <= samples; ++ii) {                                  // :171-216
        SBTV_TRY(iteration((size_t)wsteps + (size_t)(ii - 2), WS_PH_MAIN, ii));
        if ((ii & 1023) == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    SBTV_TRY(wav_chain_spectrum(ctx, wc));                                   // the residual of the last sample
    SBTV_TRY(wav_chain_rows(ctx, wc, OP_RESID, acc));
    SBTV_TRY(update(WS_PH_LAST, samples + 1, 0.0));
    ctx->calls += batch;

    std::vector<double> tr(trlen);
    std::vector<WavSapgChain> ch((size_t)batch);
    SBTV_HIP(ctx, hipMemcpyAsync(tr.data(), tr_d, sizeof(double) * trlen, hipMemcpyDeviceToHost, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(ch.data(), u.chain, sizeof(WavSapgChain) * batch, hipMemcpyDeviceToHost, ctx->stream));
    SBTV_TRY(stage_out_copy(ctx, xw_last, X, ccnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int nmean = samples - op->burnIn;
    for (int b = 0; b < batch; ++b) {
        const size_t o = (size_t)b * samples;
        tr[o] = op->th_init;                                                 // theta(1)  (:146)
        theta_eb[b] = ch[b].theta_eb;
        for (int i = 0; i < samples; ++i) {
            if (thetas) thetas[o + i] = tr[o + i];
            if (gx) gx[o + i] = tr[bs + o + i];
            if (logpi) logpi[o + i] = tr[2 * bs + o + i];
            if (tol_thetas) tol_thetas[o + i] = tr[4 * bs + o + i];
        }
        for (int i = 0; mean_thetas && i < nmean; ++i) mean_thetas[(size_t)b * nmean + i] = tr[3 * bs + o + i];
        for (int i = 0; logpi_wu && i < warmup; ++i) logpi_wu[(size_t)b * warmup + i] = tr[5 * bs + (size_t)b * wstride + i];
    }
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

// MYULA chain on the coefficients of the redundant wavelet frame at a FIXED theta, with the posterior mean / variance of its
// samples in the image and in the coefficient domain.  No entry of the reference: it is the warm-up loop of
// SALSA/SAPG_algorithm_1.m:131-141 with the closures of SALSA/run_deblur_synthesis_L1.m:135-146 (proxG = soft, g = l1,
// gradF = W' B'(B W xw - y) / sigma2), run at the caller's theta - what a user does with the theta_EB of sbtv_SAPG_wavelet.
//
// One iteration is that of wavelet_sapg.hip without the parameter update, from the pieces of wavelet_chain.hip: J synthesis
// launches, the FFT triple with OP_GRADF (its Parseval sum is ||B W X - y||^2 of the state BEFORE the step), J analysis
// launches and wav_step_kernel (the element-wise update of wav_myula_nocontract and the partial sums of |X_new|).  Nothing is reduced per iteration: the row
// pass and the step kernel leave their partial sums in a ring of up to WM_RING slots, and wav_myula_trace_kernel turns a full
// ring into gx / logpi entries in one launch, one workgroup per chain and iteration, every sum in a fixed order.
//
// Moments.  The image W X(ii) exists only inside the level-1 synthesis launch of iteration ii + 1 (or of the final residual
// pass): wav_synthesis_moments_kernel (wavelet.hip) accumulates it there, on the value it is about to store.  The
// coefficients X(ii) are in registers of the step kernel: wav_step_kernel<true> accumulates them with moments_pair.
// Unselected iterations launch the plain kernels; the chain's bits do not depend on what is accumulated.
#include <cmath>
#include <cstring>
#include <vector>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

constexpr int WM_RING = 1024;     // iterations between two trace launches (and two synchronisations)

struct WavMyulaDev {
    const double *par;           // [2][batch]: theta | sigma2
    const double *part;          // ring [slot][batch][nblk]: partial sums of |X| after the slot's step
    const double *acc;           // ring [slot][batch][3][nrb]: accumulators of the slot's row pass, q = 0: ||B W X - y||^2
    double *gx, *logpi;          // [batch][samples]
    int batch, nblk, nrb, samples;
    double parseval;
};

// The traces of the iterations ii0, ii0 + 1, ... whose partial sums sit in the ring slots 0, 1, ...: grid (batch, slots), one
// workgroup per chain and iteration.  Slot s of iteration ii holds R = ||B W X(ii-1) - y||^2 (has_r: the row pass ran before
// the step) and g = ||X(ii)||_1 (has_g: the step ran):
//     logpi(ii-1) = -R / (2 sigma2_b) - theta_b gx(ii-1) ;  gx(ii) = g
// gx(ii-1) is summed again from the slot before (the same additions in the same order as the workgroup that stores it), or,
// for slot 0, read from the trace an earlier launch wrote.  Start state: has_g only (ii0 = 1); final residual: has_r only
// (ii0 = samples + 1).
__global__ __launch_bounds__(WAV_EWB) void wav_myula_trace_kernel(WavMyulaDev u, int ii0, int has_r, int has_g) {
    __shared__ double red[4];
    const int b = blockIdx.x, s = blockIdx.y, ii = ii0 + s, S = u.samples;
    if (has_r) {
        const double *a = u.acc + ((size_t)s * u.batch + b) * 3 * u.nrb;
        double r = 0.0, gp = 0.0;
        for (int i = threadIdx.x; i < u.nrb; i += WAV_EWB) r += a[i];
        r = wav_block_sum(r, red);
        if (s > 0) {
            const double *p = u.part + ((size_t)(s - 1) * u.batch + b) * u.nblk;
            for (int i = threadIdx.x; i < u.nblk; i += WAV_EWB) gp += p[i];
            gp = wav_block_sum(gp, red);
        } else {
            gp = u.gx[(size_t)b * S + (ii - 2)];
        }
        const double f = (r * u.parseval) / (2 * u.par[u.batch + b]);
        if (threadIdx.x == 0) u.logpi[(size_t)b * S + (ii - 2)] = -f - u.par[b] * gp;
    }
    if (has_g) {
        const double *p = u.part + ((size_t)s * u.batch + b) * u.nblk;
        double g = 0.0;
        for (int i = threadIdx.x; i < u.nblk; i += WAV_EWB) g += p[i];
        g = wav_block_sum(g, red);
        if (threadIdx.x == 0) u.gx[(size_t)b * S + (ii - 1)] = g;
    }
}

inline bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_myula_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                       const double *h, int hlen, int levels, const sbtv_myula_wavelet_opts *op, const double *theta,
                       const double *sigma2, const double *xw0, const double *noise, double *gx, double *logpi,
                       double *xw_last, const sbtv_moments_opts *mo, double *post_mean, double *post_var,
                       long long *post_count, double *coef_mean, double *coef_var, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!y || !op || !theta || !sigma2 || batch < 1)
        return fail(ctx, SBTV_ERR_BADARG, "myula_wavelet: missing required argument (y, op, theta, sigma2, batch >= 1)");
    if (!taps) return fail(ctx, SBTV_ERR_MISSING_AT, "The function handle for transpose of A is missing");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    if (op->samples < 2) return fail(ctx, SBTV_ERR_BADARG, "myula_wavelet: need samples >= 2");
    if (!positive_finite(op->lambda) || !positive_finite(op->gamma))
        return fail(ctx, SBTV_ERR_BADARG, "myula_wavelet: lambda and gamma must be finite and > 0");
    for (int b = 0; b < batch; ++b)
        if (!positive_finite(theta[b]) || !positive_finite(sigma2[b]))
            return fail(ctx, SBTV_ERR_BADARG, "myula_wavelet: every theta[b] and sigma2[b] must be finite and > 0");
    if (op->chain_offset < 0) return fail(ctx, SBTV_ERR_BADARG, "myula_wavelet: chain_offset must be >= 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    const int samples = op->samples;
    const size_t P = (size_t)M * N, cnt = P * batch, dimX = P * wp.bands(), ccnt = dimX * batch;
    const bool dev = (flags & SBTV_DEVICE_PTRS) != 0;
    // the moments request: one selection for both domains
    MomReq sel{};
    const MomReq *selp = nullptr;
    if (mo) {
        if (!post_mean && !coef_mean)
            return fail(ctx, SBTV_ERR_BADARG, "myula_wavelet: moments need post_mean or coef_mean");
        if ((post_var && !post_mean) || (coef_var && !coef_mean))
            return fail(ctx, SBTV_ERR_BADARG, "myula_wavelet: post_var needs post_mean and coef_var needs coef_mean");
    } else if (post_mean || post_var || post_count || coef_mean || coef_var) {
        return fail(ctx, SBTV_ERR_BADARG, "myula_wavelet: moment outputs without moments options");
    }
    // MomReq's outputs are set per domain where the moments are finished
    SBTV_TRY(mom_resolve(ctx, "myula_wavelet", mo, 1, samples, post_mean ? post_mean : coef_mean, nullptr, nullptr, dev, &sel, &selp));
    if (selp && sel.pooled && batch > 1)
        SBTV_TRY(check_one_posterior(ctx, "myula_wavelet", y, P, taps, taille, theta, sigma2, batch, dev));
    const bool mom_img = selp && post_mean, mom_coef = selp && coef_mean;

    WavChain wc;
    SBTV_TRY(wav_chain_buffers(ctx, "wmy", wp, batch, y, xw0, noise, xw_last, flags, &wc));
    const int nblk = wc.nblk, nrb = wc.nrb;
    const int ring = samples - 1 < WM_RING ? samples - 1 : WM_RING;
    double *X = wc.X, *par = nullptr, *taps_d = nullptr, *acc = nullptr, *part = nullptr, *tr_d = nullptr, *im_mean = nullptr,
           *im_m2 = nullptr, *c_mean = nullptr, *c_m2 = nullptr;
    SBTV_TRY(ws_get_t(ctx, "wmy.acc", (size_t)ring * batch * 3 * nrb, &acc));
    SBTV_TRY(ws_get_t(ctx, "wmy.part", (size_t)ring * batch * nblk, &part));
    const size_t t2b = (size_t)taille * taille * batch, npar = 2 * (size_t)batch + t2b;
    SBTV_TRY(ws_get_t(ctx, "wmy.par", npar, &par));                          // [theta | sigma2 | taps]
    taps_d = par + 2 * (size_t)batch;
    const size_t bs = (size_t)batch * samples, trlen = 2 * bs;
    SBTV_TRY(ws_get_t(ctx, "wmy.traces", trlen, &tr_d));
    if (mom_img) {
        SBTV_TRY(ws_get_t(ctx, "wmy.im_mean", cnt, &im_mean));
        SBTV_TRY(ws_get_t(ctx, "wmy.im_m2", cnt, &im_m2));
    }
    if (mom_coef) {
        SBTV_TRY(ws_get_t(ctx, "wmy.c_mean", ccnt, &c_mean));
        SBTV_TRY(ws_get_t(ctx, "wmy.c_m2", ccnt, &c_m2));
    }
    WavMyulaDev u{};
    u.par = par; u.part = part; u.acc = acc; u.gx = tr_d; u.logpi = tr_d + bs; u.batch = batch; u.nblk = nblk; u.nrb = nrb;
    u.samples = samples; u.parseval = 1.0 / ((double)M * N);

    // constants, spectra of the PSF and of y, the start state
    {
        std::vector<double> hp(npar);
        for (int b = 0; b < batch; ++b) {
            hp[b] = theta[b];
            hp[batch + b] = sigma2[b];
        }
        for (size_t q = 0; q < t2b; ++q) hp[2 * (size_t)batch + q] = taps[q];
        SBTV_HIP(ctx, hipMemcpyAsync(par, hp.data(), sizeof(double) * npar, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(tr_d, 0, sizeof(double) * trlen, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));                    // the staging vector goes out of scope
    }
    SBTV_TRY(psf_spectrum(ctx, wc.op.fp, taps_d, taille, wc.op.Hs));
    SBTV_TRY(wav_chain_start(ctx, wc));
    // the traces of `slots` ring slots, the first of them iteration ii0
    auto trace = [&](int slots, int ii0, int has_r, int has_g) -> int {
        hipLaunchKernelGGL(wav_myula_trace_kernel, dim3(batch, slots), dim3(WAV_EWB), 0, ctx->stream, u, ii0, has_r, has_g);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };
    SBTV_TRY(wav_abs_sum(ctx, wc, part));
    SBTV_TRY(trace(1, 1, 0, 1));                                             // gx(1)
    if (mom_coef && mom_sample_of(selp, 1)) SBTV_TRY(moments_seed(ctx, X, c_mean, c_m2, dimX, batch));        // iteration 1

    const WavStepPar sp{par, par + batch, 1};
    // W' B'(B W X - y) -> G and ||B W X - y||^2 -> the slot's accumulators (OP_GRADF), or the sum alone (OP_RESID); X is
    // sample number `of` of the chain: its image is accumulated while the level-1 synthesis stores it
    auto operator_pass = [&](int rows_op, int slot, int of) -> int {
        const MomArgs ma{im_mean, im_m2, mom_img ? mom_sample_of(selp, of) : 0, nullptr, 1, 1};
        SBTV_TRY(wav_chain_spectrum(ctx, wc, &ma));
        return wav_chain_rows(ctx, wc, rows_op, acc + (size_t)slot * batch * 3 * nrb);
    };
    int filled = 0;                                                          // ring slots waiting for the trace kernel
    for (int ii = 2; ii <= samples; ++ii) {                                  // SAPG_algorithm_1.m:131-141 at theta_b
        const int slot = filled;
        SBTV_TRY(operator_pass(OP_GRADF, slot, ii - 1));
        const RngArgs r{op->seed, (unsigned)(ii - 2), (unsigned)op->chain_offset, nullptr};
        const MomArgs mc{c_mean, c_m2, mom_coef ? mom_sample_of(selp, ii) : 0, nullptr, 1, 1};
        SBTV_TRY(wav_chain_step(ctx, wc, sp, op->gamma, op->lambda, r, part + (size_t)slot * batch * nblk, &mc));
        ctx->calls += 2 * (long long)batch;
        if (++filled == ring || ii == samples) {
            SBTV_TRY(trace(filled, ii - filled + 1, 1, 1));
            if (filled == WM_RING) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            filled = 0;
        }
    }
    SBTV_TRY(operator_pass(OP_RESID, 0, samples));                           // the residual (and the image) of the last sample
    SBTV_TRY(trace(1, samples + 1, 1, 0));
    ctx->calls += batch;

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
    SBTV_TRY(stage_out_copy(ctx, xw_last, X, ccnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < bs; ++i) {
        if (gx) gx[i] = tr[i];
        if (logpi) logpi[i] = tr[bs + i];
    }
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

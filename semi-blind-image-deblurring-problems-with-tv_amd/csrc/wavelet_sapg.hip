// Empirical-Bayes estimate of the regularisation parameter theta of the wavelet-l1 prior: the MYULA chain
// on the coefficients of the redundant wavelet frame and the log-scale stochastic update of SALSA/SAPG_algorithm_1.m:120-216,
// as SALSA/run_deblur_synthesis_L1.m:125-156 sets them up (proxG = soft, g = l1, gradF = W' B'(B W xw - y) / sigma2).  Only the
// theta part of SAPG_algorithm_1.m is built: its second parameter `tau` needs op.to_init, op.grad_t and a two-argument gradF
// that the script never defines; csrc/wavelet_sapg_sb.hip builds that part with the PSF parameters as tau.
//
// The loop is device-resident.  The array-sized state is the chain X [batch][3J+1][M N] and the gradient; the prox is never
// stored: wav_myula_kernel recomputes soft(X, lambda theta) from X and the theta the reference formed it with, which lags
// one iteration.  One iteration: J synthesis launches, the FFT triple with OP_GRADF (whose Parseval sum is ||B W X - y||^2 of
// the state BEFORE the step), J analysis launches, wav_myula_kernel (the whole element-wise update and the partial sums of
// |X_new|) and wav_sapg_update_kernel (one workgroup per chain: the sums in a fixed order, eta / theta, the traces).  The
// residual of sample ii is the one the next iteration computes anyway, so logpi(ii) is completed one iteration late; the last
// sample costs one extra synthesis + forward transform + OP_RESID.
#include <cmath>
#include <vector>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

constexpr int WSB = WAV_EWB;      // lanes per workgroup of the kernels below

// what the update kernel keeps per chain between two iterations
struct WavSapgChain {
    double eta;        // eta(ii-1)
    double th_prev;    // theta(ii-2): the theta the prox of the next MYULA step is formed with (theta(1) at ii = 2)
    double th_cur;     // theta(ii-1)
    double g_last;     // ||X||_1 of the current sample
    double sum_eta;    // sum of eta(burnIn .. ii-1)
    double n_eta;      // its number of terms
    double theta_eb;   // set by the last phase
    double pad;
};

// traces of all chains on the device: [batch][samples] each, wu [batch][wstride]
struct WavSapgTraces {
    double *thetas, *gx, *logpi, *mean, *tol, *wu;
};

struct WavSapgDev {
    WavSapgChain *chain;         // [batch]
    const double *part;          // [batch][nblk] partial sums of |X_new| (wav_myula_kernel / wav_l1_kernel)
    const double *acc;           // [batch][3][nrb] accumulators of the row pass, q = 0: ||B W X - y||^2 (unscaled)
    int nblk, nrb, samples, warmup, wstride, burnIn;
    double parseval, sigma2, dimX, min_eta, max_eta;
    WavSapgTraces tr;
};

enum { WS_PH_START = 0, WS_PH_WARMUP = 1, WS_PH_MAIN = 2, WS_PH_LAST = 3 };

// ||X||_1 of the start state: partials [batch][gridDim.x]
__global__ __launch_bounds__(WSB) void wav_l1_kernel(const double *__restrict__ X, size_t dimX,
                                                      double *__restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const double *x = X + (size_t)b * dimX;
    double a = 0.0;
    for (size_t q = (size_t)blockIdx.x * WSB + threadIdx.x; q < dimX / 2; q += (size_t)gridDim.x * WSB) {
        const double2 v = *reinterpret_cast<const double2 *>(x + 2 * q);
        a += fabs(v.x) + fabs(v.y);
    }
    a = wav_block_sum(a, red);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = a;
}

// One MYULA step of every chain (SAPG_algorithm_1.m:133,174) on the coefficients, two per lane (dimX is even: an odd pixel
// count is refused):
//     prox = soft(X, lambda theta)   with the theta of the iteration before (chain[b].th_prev)
//     X    = X + gamma (prox - X) / lambda - gamma G / sigma2 + sqrt(2 gamma) Z
// G = W' B'(B W X - y).  Z: injected normals in the layout of X, or null: pair q of chain b draws
// philox_normal_pair(q, step, chain0 + b, seed).  X and G are read once, X is written once; part [batch][gridDim.x]
// receives the workgroup's sum of |X_new|.
__global__ __launch_bounds__(WSB) void wav_myula_kernel(double *__restrict__ X, const double *__restrict__ G,
                                                         const double *__restrict__ Z,
                                                         const WavSapgChain *__restrict__ chain, double gam, double lamb,
                                                         double s2, double sq2g, size_t dimX, RngArgs rng,
                                                         double *__restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * dimX;
    const double T = lamb * chain[b].th_prev;
    double a = 0.0;
    for (size_t q = (size_t)blockIdx.x * WSB + threadIdx.x; q < dimX / 2; q += (size_t)gridDim.x * WSB) {
        const size_t o = base + 2 * q;
        const double2 xv = *reinterpret_cast<const double2 *>(X + o);
        const double2 gv = *reinterpret_cast<const double2 *>(G + o);
        const double2 zv = Z ? *reinterpret_cast<const double2 *>(Z + o)
                             : philox_normal_pair(q, rng.step, rng.chain0 + (unsigned)b, rng.seed);
        double2 r;
        r.x = wav_myula_nocontract(xv.x, gv.x, zv.x, T, gam, lamb, s2, sq2g);
        r.y = wav_myula_nocontract(xv.y, gv.y, zv.y, T, gam, lamb, s2, sq2g);
        *reinterpret_cast<double2 *>(X + o) = r;
        a += fabs(r.x) + fabs(r.y);
    }
    a = wav_block_sum(a, red);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = a;
}

// End of an iteration, one workgroup per chain.  R = ||B W X - y||^2 of the state before this iteration's step (the row
// pass), g = ||X_new||_1 (the step's partials), both summed in a fixed order.
//   WS_PH_START: no step yet, only g of the start state is booked (the partials of wav_l1_kernel)
//   every other phase: the log-density of the PREVIOUS sample is completed with R (SAPG_algorithm_1.m:136,166,190)
//   WS_PH_MAIN, iteration ii: eta / theta (:180-182), gx (:191), tol_thetas / mean_thetas (:199-211)
//   WS_PH_LAST: nothing was stepped; R belongs to sample `samples`; theta_EB (:226)
__global__ __launch_bounds__(WSB) void wav_sapg_update_kernel(WavSapgDev u, int phase, int ii, double delta) {
    __shared__ double red[4];
    const int b = blockIdx.x, S = u.samples;
    double r = 0.0, g = 0.0;
    if (phase != WS_PH_START) {
        for (int i = threadIdx.x; i < u.nrb; i += WSB) r += u.acc[(size_t)b * 3 * u.nrb + i];
        r = wav_block_sum(r, red);
    }
    if (phase != WS_PH_LAST) {
        for (int i = threadIdx.x; i < u.nblk; i += WSB) g += u.part[(size_t)b * u.nblk + i];
        g = wav_block_sum(g, red);
    }
    if (threadIdx.x != 0) return;
    WavSapgChain c = u.chain[b];
    const double f = (r * u.parseval) / (2 * u.sigma2);
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
    const double etaii = c.eta + delta * (u.dimX / c.th_cur - g) * exp(c.eta);   // :180
    const double eta = fmin(fmax(etaii, u.min_eta), u.max_eta);                  // :181
    const double th = exp(eta);                                                  // :182
    u.tr.thetas[(size_t)b * S + (ii - 1)] = th;
    u.tr.gx[(size_t)b * S + (ii - 2)] = g;                                       // :191
    const double nan = __builtin_nan("");
    const double m0 = c.n_eta > 0.0 ? exp(c.sum_eta / c.n_eta) : nan;            // exp(mean(eta(burnIn:ii-1))), empty: NaN
    if (ii >= u.burnIn) {
        c.sum_eta += eta;
        c.n_eta += 1.0;
    }
    const double m1 = c.n_eta > 0.0 ? exp(c.sum_eta / c.n_eta) : nan;
    u.tr.tol[(size_t)b * S + (ii - 1)] = fabs(m1 - m0) / m0;                     // :199-200
    if (ii > u.burnIn) u.tr.mean[(size_t)b * S + (ii - u.burnIn - 1)] = m1;      // :211
    c.eta = eta;
    c.th_prev = c.th_cur;
    c.th_cur = th;
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
    if (taille < 1 || taille > 15 || taille > M || taille > N) return fail(ctx, SBTV_ERR_PSF, "Mask does not fit inside array");
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    if (op->samples < 2 || op->warmup < 0 || op->burnIn < 1 || op->burnIn > op->samples)
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: need samples >= 2, warmup >= 0, 1 <= burnIn <= samples");
    if (!(op->lambda > 0.0) || !(op->gamma > 0.0) || !(op->sigma2 > 0.0))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: lambda, gamma and sigma2 must be > 0");
    if (!(op->min_th > 0.0) || !(op->min_th <= op->th_init) || !(op->th_init <= op->max_th))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: need 0 < min_th <= th_init <= max_th");
    if (op->chain_offset < 0) return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet: chain_offset must be >= 0");
    if (((size_t)M * N) & 1)
        return fail(ctx, SBTV_ERR_SIZE, "this entry point needs an even number of pixels (its element-wise passes move two per lane)");
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    FftPlan fp;
    SBTV_TRY(fft_plan(ctx, M, N, batch, &fp));
    const int samples = op->samples, warmup = op->warmup, wsteps = warmup > 0 ? warmup - 1 : 0, wstride = warmup > 0 ? warmup : 1;
    const size_t P = (size_t)M * N, cnt = P * batch, dimX = P * wp.bands(), ccnt = dimX * batch, spec = fp.u_img;
    const int nblk = wav_ew_blocks(dimX), nrb = fft_rows_blocks(fp);
    const bool noise_host = noise && !(flags & SBTV_DEVICE_PTRS);

    const double *yd = nullptr, *x0d = nullptr;
    SBTV_TRY(stage_in(ctx, "wsapg.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "wsapg.G", xw0, ccnt, flags, &x0d));             // staged where the gradient goes later
    double *X = nullptr, *G = nullptr, *img = nullptr, *Z = nullptr, *taps_d = nullptr, *acc = nullptr, *part = nullptr,
           *tr_d = nullptr;
    double2 *S = nullptr, *Hs = nullptr, *Ys = nullptr;
    WavSapgDev u{};
    SBTV_TRY(stage_out_buf(ctx, "wsapg.X", xw_last, ccnt, flags, &X));
    SBTV_TRY(ws_get_t(ctx, "wsapg.G", ccnt, &G));
    SBTV_TRY(ws_get_t(ctx, "wsapg.img", cnt, &img));
    if (noise_host) SBTV_TRY(ws_get_t(ctx, "wsapg.Z", ccnt, &Z));
    SBTV_TRY(ws_get_t(ctx, "wsapg.S", (size_t)batch * fp.s_img, &S));
    SBTV_TRY(ws_get_t(ctx, "wsapg.H", spec * batch, &Hs));
    SBTV_TRY(ws_get_t(ctx, "wsapg.Y", spec * batch, &Ys));
    SBTV_TRY(ws_get_t(ctx, "wsapg.acc", (size_t)batch * 3 * nrb, &acc));
    SBTV_TRY(ws_get_t(ctx, "wsapg.part", (size_t)batch * nblk, &part));
    SBTV_TRY(ws_get_t(ctx, "wsapg.taps", (size_t)taille * taille * batch, &taps_d));
    SBTV_TRY(ws_get_t(ctx, "wsapg.chain", (size_t)batch, &u.chain));
    const size_t bs = (size_t)batch * samples, trlen = 5 * bs + (size_t)batch * wstride;
    SBTV_TRY(ws_get_t(ctx, "wsapg.traces", trlen, &tr_d));
    u.tr = WavSapgTraces{tr_d, tr_d + bs, tr_d + 2 * bs, tr_d + 3 * bs, tr_d + 4 * bs, tr_d + 5 * bs};
    u.part = part; u.acc = acc; u.nblk = nblk; u.nrb = nrb; u.samples = samples; u.warmup = warmup; u.wstride = wstride;
    u.burnIn = op->burnIn; u.parseval = 1.0 / ((double)M * N); u.sigma2 = op->sigma2; u.dimX = (double)dimX;
    u.min_eta = log(op->min_th); u.max_eta = log(op->max_th);

    // constants, spectra of the PSF and of y, the start state
    const double eta_init = log(op->th_init);                                // :101
    {
        const WavSapgChain c0{eta_init, op->th_init, op->th_init, 0.0, op->burnIn == 1 ? eta_init : 0.0,
                              op->burnIn == 1 ? 1.0 : 0.0, 0.0, 0.0};
        std::vector<WavSapgChain> ch((size_t)batch, c0);
        SBTV_HIP(ctx, hipMemcpyAsync(u.chain, ch.data(), sizeof(WavSapgChain) * batch, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(taps_d, taps, sizeof(double) * taille * taille * batch, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(tr_d, 0, sizeof(double) * trlen, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));                    // the staging vector goes out of scope
    }
    SBTV_TRY(psf_spectrum(ctx, fp, taps_d, taille, Hs));
    {
        RowsArgs a{};
        a.dir_fwd = 1;
        SBTV_TRY(fft_cols_fwd(ctx, fp, yd, nullptr, S));
        SBTV_TRY(fft_rows(ctx, fp, S, S, a));
        SBTV_TRY(spec_unpack(ctx, fp, S, Ys));
    }
    if (x0d) {
        if (x0d != X) SBTV_HIP(ctx, hipMemcpyAsync(X, x0d, sizeof(double) * ccnt, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        SBTV_TRY(wav_analysis(ctx, wp, yd, X, batch));                       // op.X0 = WT(y)  (run_deblur_synthesis_L1.m:153)
    }
    const dim3 grid(nblk, batch);
    if (wsteps == 0) {
        // logPiTraceX(1) needs g of the start state (:166); after a warm-up the last warm-up step has left it
        hipLaunchKernelGGL(wav_l1_kernel, grid, dim3(WSB), 0, ctx->stream, (const double *)X, dimX, part);
        hipLaunchKernelGGL(wav_sapg_update_kernel, dim3(batch), dim3(WSB), 0, ctx->stream, u, (int)WS_PH_START, 1, 0.0);
        SBTV_HIP(ctx, hipGetLastError());
    }
    const double inv_scale = 1.0 / ((double)fp.n1 * N), gam = op->gamma, lamb = op->lambda, sq2g = sqrt(2 * gam);
    RowsArgs ra{};
    ra.dir_fwd = 1;
    ra.H = Hs;
    ra.Y = Ys;
    ra.acc = acc;
    // W' B'(B W X - y) -> G and ||B W X - y||^2 -> acc, or (resid_only) the sum alone
    auto operator_pass = [&](bool resid_only) -> int {
        SBTV_TRY(wav_synthesis(ctx, wp, X, img, batch));
        SBTV_TRY(fft_cols_fwd(ctx, fp, img, nullptr, S));
        ra.dir_inv = resid_only ? 0 : 1;
        ra.op = resid_only ? OP_RESID : OP_GRADF;
        SBTV_TRY(fft_rows(ctx, fp, S, resid_only ? nullptr : S, ra));
        if (resid_only) return 0;
        SBTV_TRY(fft_cols_inv(ctx, fp, S, img, inv_scale));
        return wav_analysis(ctx, wp, img, G, batch);
    };
    // MYULA step number `step` of the call (warm-up steps first, as the noise array is laid out) and its update
    auto iteration = [&](size_t step, int phase, int ii) -> int {
        SBTV_TRY(operator_pass(false));
        const double *zd = nullptr;
        if (noise_host) {
            SBTV_HIP(ctx, hipMemcpyAsync(Z, noise + step * ccnt, sizeof(double) * ccnt, hipMemcpyHostToDevice, ctx->stream));
            zd = Z;
        } else if (noise) {
            zd = noise + step * ccnt;
        }
        const RngArgs r{op->seed, (unsigned)step, (unsigned)op->chain_offset, nullptr};
        hipLaunchKernelGGL(wav_myula_kernel, grid, dim3(WSB), 0, ctx->stream, X, (const double *)G, zd,
                           (const WavSapgChain *)u.chain, gam, lamb, op->sigma2, sq2g, dimX, r, part);
        // delta(ii) of :111
        const double delta = phase == WS_PH_MAIN ? op->d_scale * (pow((double)ii, -op->d_exp) / (double)dimX) : 0.0;
        hipLaunchKernelGGL(wav_sapg_update_kernel, dim3(batch), dim3(WSB), 0, ctx->stream, u, phase, ii, delta);
        SBTV_HIP(ctx, hipGetLastError());
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
    SBTV_TRY(operator_pass(true));                                           // the residual of the last sample
    hipLaunchKernelGGL(wav_sapg_update_kernel, dim3(batch), dim3(WSB), 0, ctx->stream, u, (int)WS_PH_LAST, samples + 1, 0.0);
    SBTV_HIP(ctx, hipGetLastError());
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

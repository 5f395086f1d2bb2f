// Semi-blind empirical Bayes for the wavelet-l1 prior: theta, the PSF parameters and sigma2 estimated
// together from one MYULA chain on the coefficients of the redundant wavelet frame.  It is SALSA/SAPG_algorithm_1.m with BOTH
// of its parameters: the log-scale theta step of sbtv_SAPG_wavelet (csrc/wavelet_sapg.hip) and the projected gradient step
// of its second parameter `tau` (:105-108,117,185-186), here the PSF parameters p, with the closures the script
// run_deblur_synthesis_L1.m never defines taken from the TV half of this library (op.grad_t = <dB/dp W X, B W X - y> / sigma2,
// taps and derivative taps of psf_taps.inc, scaled as SAPG/SAPG_algorithm_laplace.m:172-186, which also gives the sigma2 step).
//
// The loop is device-resident.  One iteration ii (launch list of csrc/sapg.hip's device loop, on the coefficients):
//   row pass OP_GRADF on the column spectrum S of W X that the previous iteration left, with H of p(ii-1); inverse column
//     pass; J analysis launches -> G = W' B'(B W X - y)
//   wav_step_kernel (wavelet_chain.hip, which holds what the three chain drivers share): sigma2(ii-1) and the lagging theta
//     read from the chain block in device memory; partial sums of |X_new|
//   J synthesis launches, forward column pass -> S; row pass OP_GRAD without store, H / D1 / D2 of p(ii-1): ||B W X - y||^2
//     and the two <dB W X, r> sums of the NEW sample per row block.  The residual of sample ii is known in iteration ii:
//     no log-density is completed late, the last sample needs no extra pass.
//   wav_sb_update_kernel, one workgroup per chain: every sum in a fixed order, eta / theta, p, sigma2 with their clamps, the
//     burn-in sums, traces; with a free PSF parameter also the taps and derivative taps of p(ii), normalised in MATLAB's
//     column-major summation order (all chains in parallel: one workgroup each)
//   psf_spectrum_sets for H, D1 (and D2 for a two-parameter family), only when a PSF parameter can move.
// With every PSF parameter fixed nothing is computed from taps on the device and no spectrum is rebuilt after the start; the
// start spectra come from host taps (sbtv_psf_taps), staged once.
#include <cmath>
#include <vector>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

constexpr int WB_TMAX = 15 * 15;  // taps of the largest mask (one lane each in the update kernel)

// what the update kernel keeps per chain between two iterations
struct WavSbChain {
    double eta;        // eta(ii-1)
    double th_prev;    // theta(ii-2): the theta the prox of the next MYULA step is formed with (theta(1) at ii = 2)
    double th_cur;     // theta(ii-1)
    double p0, p1;     // p(ii-1)
    double sig2;       // sigma2(ii-1)
    double sum_eta, sum_p0, sum_p1, sum_s;   // sums over burnIn .. ii-1
    double n_sum;      // their number of terms
    double eb[4];      // theta_EB, p0_EB, p1_EB, sigma2_EB (set by the last iteration)
    double pad;
};

// traces of all chains on the device: [batch][samples] each, ps / tol_ps / mean_ps [batch][2][samples], grads
// [batch][3][samples], wu [batch][wstride]
struct WavSbTraces {
    double *thetas, *sigmas, *gx, *logpi, *tol_th, *mean_th, *ps, *tol_ps, *mean_ps, *grads, *wu;
};

struct WavSbDev {
    WavSbChain *chain;           // [batch]
    const double *part;          // [batch][nblk] partial sums of |X_new| (wav_chain_step / wav_abs_sum)
    const double *acc;           // [batch][3][nrb] accumulators of the OP_GRAD row pass (unscaled)
    double *par;                 // [taps | d0 | d1], each [batch][taille^2]
    int nblk, nrb, samples, warmup, wstride, burnIn;
    int kind, taille, npar, params_move, fix_p0, fix_p1, fix_sigma;
    double parseval, dimX, npix, min_eta, max_eta, th_init;
    double g0_scale;             // 2 for Moffat: utils/diff_moffat_alpha.m is HALF the derivative of psf_moffat.m (below)
    double c_p0, c_p1, c_sigma, p_min0, p_max0, p_min1, p_max1, p_true0, p_true1, s_lo, s_hi, sigma2_init, phi;
    WavSbTraces tr;
};

enum { WB_PH_START = 0, WB_PH_WARMUP = 1, WB_PH_MAIN = 2 };

// mean of a running sum; NaN for an empty window, like MATLAB's mean of an empty range
__device__ __forceinline__ double wb_mean(double s, double n) { return n > 0.0 ? s / n : __builtin_nan(""); }

// End of an iteration, one workgroup per chain.  The OP_GRAD row pass has left, per row block, ||B W X - y||^2 and the two
// <dB/dp_q W X, B W X - y> sums of the sample the step kernel just wrote (PSF parameters p(ii-1)); the step kernel (or
// wav_abs_sum for the start state) has left the partial sums of |X|.  All four are summed here in a fixed order.
//   WB_PH_START : logpi(1) of the start state                                                  (SAPG_algorithm_1.m:166)
//   WB_PH_WARMUP: logpi_wu(ii) (:136), and logpi(1) again: the last warm-up sample is the start of the main loop
//   WB_PH_MAIN  : iteration ii: eta / theta (:180-182), p (:185-186, SAPG_algorithm_laplace.m:172-178), sigma2
//                 (SAPG_algorithm_laplace.m:181-186), logpi / gx (:190-191), tol / mean entries (:199-213); at ii = samples
//                 the EB estimates (:226,236); with a free PSF parameter the taps and derivative taps of p(ii)
__global__ __launch_bounds__(WAV_EWB) void wav_sb_update_kernel(WavSbDev u, int phase, int ii, double delta) {
    __shared__ double red[4];
    __shared__ double sf[WB_TMAX], se0[WB_TMAX], se1[WB_TMAX], spar[3], ssum[3];
    const int b = blockIdx.x, S = u.samples, tid = threadIdx.x;
    const double *acc = u.acc + (size_t)b * 3 * u.nrb;
    double r = 0.0, d0 = 0.0, d1 = 0.0, g = 0.0;
    for (int i = tid; i < u.nrb; i += WAV_EWB) r += acc[i];
    r = wav_block_sum(r, red);
    for (int i = tid; i < u.nblk; i += WAV_EWB) g += u.part[(size_t)b * u.nblk + i];
    g = wav_block_sum(g, red);
    if (phase == WB_PH_MAIN) {
        for (int i = tid; i < u.nrb; i += WAV_EWB) d0 += acc[u.nrb + i];
        d0 = wav_block_sum(d0, red);
        if (u.npar > 1) {
            for (int i = tid; i < u.nrb; i += WAV_EWB) d1 += acc[2 * (size_t)u.nrb + i];
            d1 = wav_block_sum(d1, red);
        }
    }
    if (tid == 0) {
        WavSbChain c = u.chain[b];
        const double s = c.sig2;
        const double R = r * u.parseval;
        const double lp = -(R / (2 * s)) - c.th_cur * g;     // logPi(X, theta(ii-1), p(ii-1), sigma2(ii-1))
        if (phase != WB_PH_MAIN) {
            if (phase == WB_PH_WARMUP) u.tr.wu[(size_t)b * u.wstride + (ii - 1)] = lp;                    // :136
            u.tr.logpi[(size_t)b * S] = lp;                                                               // :166
        } else {
            const size_t o = (size_t)b * S, i0 = (size_t)ii - 1;
            u.tr.logpi[o + i0] = lp;                                                                      // :190
            u.tr.gx[o + i0 - 1] = g;                                                                      // :191
            const WavThetaStep t = wav_theta_step(c.eta, c.th_cur, g, delta, u.dimX, u.min_eta, u.max_eta, ii >= u.burnIn,
                                                  c.sum_eta, c.n_sum);                            // :180-182,199-211
            // op.grad_t of the two PSF parameters and the sigma2 gradient (SAPG_algorithm_laplace.m:170,181)
            const double G0 = u.g0_scale * ((d0 * u.parseval) / s);
            const double G1 = u.npar > 1 ? (d1 * u.parseval) / s : 0.0;
            const double Gs = R / (2 * s * s) - u.npix / (2 * s);
            double q0 = u.fix_p0 ? u.p_true0 : c.p0 - u.c_p0 * delta * G0;                               // :185
            q0 = fmin(fmax(q0, u.p_min0), u.p_max0);                                                      // :186
            double q1 = c.p1;
            if (u.npar > 1) {
                q1 = u.fix_p1 ? u.p_true1 : c.p1 - u.c_p1 * delta * G1;
                q1 = fmin(fmax(q1, u.p_min1), u.p_max1);
            }
            double sn = u.fix_sigma ? u.sigma2_init : s + u.c_sigma * delta * Gs;
            sn = fmin(fmax(sn, u.s_lo), u.s_hi);
            u.tr.thetas[o + i0] = t.th;
            u.tr.sigmas[o + i0] = sn;
            u.tr.ps[2 * o + i0] = q0;
            u.tr.ps[2 * o + S + i0] = q1;
            u.tr.grads[3 * o + i0] = G0;
            u.tr.grads[3 * o + S + i0] = G1;
            u.tr.grads[3 * o + 2 * (size_t)S + i0] = Gs;
            // relative change of the running means (:199-205) and the means themselves (:209-213); the theta step has
            // counted the terms of all four sums
            const double a00 = wb_mean(c.sum_p0, c.n_sum), a10 = wb_mean(c.sum_p1, c.n_sum);
            c.sum_eta = t.sum_eta;
            c.n_sum = t.n_eta;
            if (ii >= u.burnIn) {
                c.sum_p0 += q0;
                c.sum_p1 += q1;
                c.sum_s += sn;
            }
            const double a01 = wb_mean(c.sum_p0, c.n_sum), a11 = wb_mean(c.sum_p1, c.n_sum);
            u.tr.tol_th[o + i0] = t.tol;
            u.tr.tol_ps[2 * o + i0] = fabs(a01 - a00) / a00;
            if (u.npar > 1) u.tr.tol_ps[2 * o + S + i0] = fabs(a11 - a10) / a10;
            if (ii > u.burnIn) {
                u.tr.mean_th[o + (ii - u.burnIn - 1)] = t.mean;
                u.tr.mean_ps[2 * o + (ii - u.burnIn - 1)] = a01;
                if (u.npar > 1) u.tr.mean_ps[2 * o + S + (ii - u.burnIn - 1)] = a11;
            }
            c.eta = t.eta;
            c.th_prev = c.th_cur;
            c.th_cur = t.th;
            c.p0 = q0;
            c.p1 = q1;
            c.sig2 = sn;
            if (ii == S) {
                c.eb[0] = exp(c.sum_eta / c.n_sum);                                                       // :226
                c.eb[1] = c.sum_p0 / c.n_sum;                                                             // :236
                c.eb[2] = u.npar > 1 ? c.sum_p1 / c.n_sum : c.p1;
                c.eb[3] = c.sum_s / c.n_sum;
            }
            u.chain[b] = c;
            spar[0] = q0;
            spar[1] = u.kind == SBTV_PSF_LAPLACE ? 0.0 : q1;
            spar[2] = u.kind == SBTV_PSF_GAUSSIAN ? u.phi : 0.0;
        }
    }
    if (phase != WB_PH_MAIN || !u.params_move) return;
    // taps and derivative taps of p(ii) (sbtv_psf_taps): one lane per tap, the sums on lane 0 in MATLAB's column-major order
    __syncthreads();
    const int t2 = u.taille * u.taille;
    if (tid < t2) {
        const double pv[3] = {spar[0], spar[1], spar[2]};
        psf_taps_point(u.kind, u.taille, pv, tid, &sf[tid], &se0[tid], &se1[tid]);
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0, a0 = 0, a1 = 0;
        for (int q = 0; q < t2; ++q) {
            a += sf[q];
            a0 += se0[q];
            a1 += se1[q];
        }
        ssum[0] = a;
        ssum[1] = a0;
        ssum[2] = a1;
    }
    __syncthreads();
    if (tid < t2) {
        const double a = ssum[0];
        const size_t set = (size_t)t2 * gridDim.x, o = (size_t)b * t2 + tid;
        u.par[o] = sf[tid] / a;
        u.par[set + o] = (se0[tid] * a - sf[tid] * ssum[1]) / (a * a);
        u.par[2 * set + o] = (se1[tid] * a - sf[tid] * ssum[2]) / (a * a);
    }
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_SAPG_wavelet_semiblind(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *h, int hlen,
                                int levels, const sbtv_sapg_wavelet_sb_opts *op, const double *p_start, const double *xw0,
                                const double *noise, double *thetas, double *ps, double *sigmas, double *gx, double *logpi,
                                double *logpi_wu, double *grads, double *mean_thetas, double *tol_thetas, double *mean_ps,
                                double *tol_ps, double *eb, double *xw_last, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!y || !op || !eb || batch < 1) return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: missing required argument");
    if (op->kind < 0 || op->kind > 2) return fail(ctx, SBTV_ERR_PSF, "SAPG_wavelet_semiblind: unknown PSF kind");
    const int taille = op->psf_size;
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    if (op->samples < 2 || op->warmup < 0 || op->burnIn < 1 || op->burnIn > op->samples)
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: need samples >= 2, warmup >= 0, 1 <= burnIn <= samples");
    if (!(op->lambda > 0.0) || !(op->gamma > 0.0) || !(op->sigma2 > 0.0))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: lambda, gamma and sigma2 must be > 0");
    if (!(op->min_th > 0.0) || !(op->min_th <= op->th_init) || !(op->th_init <= op->max_th))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: need 0 < min_th <= th_init <= max_th");
    if (op->chain_offset < 0) return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: chain_offset must be >= 0");
    const int npar = op->kind == SBTV_PSF_LAPLACE ? 1 : 2;
    const bool fixq[2] = {op->fix_p[0] != 0, npar < 2 || op->fix_p[1] != 0};
    // start values of the PSF parameters: one pair per chain (p_start) or op->p_init for every chain
    std::vector<double> pinit(2 * (size_t)batch);
    for (int b = 0; b < batch; ++b)
        for (int q = 0; q < 2; ++q) pinit[2 * (size_t)b + q] = p_start ? p_start[2 * (size_t)b + q] : op->p_init[q];
    for (int q = 0; q < npar; ++q) {
        if (!(op->c_p[q] >= 0.0) || !std::isfinite(op->c_p[q]))
            return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: c_p must be finite and >= 0");
        if (fixq[q]) continue;
        for (int b = 0; b < batch; ++b) {
            const double p0 = pinit[2 * (size_t)b + q];
            if (!(op->p_min[q] > 0.0) || !(op->p_min[q] <= p0) || !(p0 <= op->p_max[q]))
                return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: a free PSF parameter needs 0 < p_min <= p_init <= p_max");
        }
    }
    if (!(op->c_sigma >= 0.0) || !std::isfinite(op->c_sigma))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: c_sigma must be finite and >= 0");
    if (!op->fix_sigma && (!(op->sigma2_min > 0.0) || !(op->sigma2_min <= op->sigma2) || !(op->sigma2 <= op->sigma2_max)))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_wavelet_semiblind: free sigma2 needs 0 < sigma2_min <= sigma2 <= sigma2_max");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    const size_t t2 = (size_t)taille * taille;
    // taps and derivative taps of the start parameters, on the host (sbtv_psf_taps): [taps | d0 | d1], each [batch][t2]
    std::vector<double> par_h(3 * t2 * batch, 0.0);
    for (int b = 0; b < batch; ++b) {
        const double pv[3] = {pinit[2 * (size_t)b], npar > 1 ? pinit[2 * (size_t)b + 1] : 0.0,
                              op->kind == SBTV_PSF_GAUSSIAN ? op->phi : 0.0};
        const int rc = sbtv_psf_taps(op->kind, taille, pv, par_h.data() + b * t2, par_h.data() + (batch + b) * t2,
                                     par_h.data() + (2 * (size_t)batch + b) * t2);
        if (rc != 0) return fail(ctx, rc, "SAPG_wavelet_semiblind: PSF parameters out of range");
    }
    // A PSF parameter can move if it is free, or fixed at a p_true that is not where it starts (then p(1) = p_init and
    // p(ii >= 2) = p_true: one rebuild would do, the general path is taken)
    bool params_move = false;
    for (int q = 0; q < npar; ++q) {
        if (!fixq[q]) params_move = true;
        const double pt = fmin(fmax(op->p_true[q], op->p_min[q]), op->p_max[q]);
        for (int b = 0; b < batch && fixq[q]; ++b)
            if (!(pinit[2 * (size_t)b + q] == pt)) params_move = true;
    }

    WavChain wc;
    SBTV_TRY(wav_chain_buffers(ctx, "wsb", wp, batch, y, xw0, noise, xw_last, flags, &wc));
    const int samples = op->samples, warmup = op->warmup, wsteps = warmup > 0 ? warmup - 1 : 0, wstride = warmup > 0 ? warmup : 1;
    const size_t P = wc.P, dimX = wc.dimX, ccnt = wc.ccnt, spec = wc.op.fp.u_img;
    double *X = wc.X, *acc = nullptr, *part = nullptr, *tr_d = nullptr;
    double2 *D1s = nullptr, *D2s = nullptr;
    WavSbDev u{};
    SBTV_TRY(ws_get_t(ctx, "wsb.D1", spec * batch, &D1s));
    // a one-parameter PSF (Laplace) has one derivative spectrum: the second one the row pass reads IS the first (sapg.hip)
    if (npar > 1) SBTV_TRY(ws_get_t(ctx, "wsb.D2", spec * batch, &D2s));
    else D2s = D1s;
    SBTV_TRY(ws_get_t(ctx, "wsb.acc", (size_t)batch * 3 * wc.nrb, &acc));
    SBTV_TRY(ws_get_t(ctx, "wsb.part", (size_t)batch * wc.nblk, &part));
    SBTV_TRY(ws_get_t(ctx, "wsb.par", 3 * t2 * batch, &u.par));
    SBTV_TRY(ws_get_t(ctx, "wsb.chain", (size_t)batch, &u.chain));
    const size_t bs = (size_t)batch * samples, trlen = 15 * bs + (size_t)batch * wstride;
    SBTV_TRY(ws_get_t(ctx, "wsb.traces", trlen, &tr_d));
    u.tr = WavSbTraces{tr_d,          tr_d + bs,     tr_d + 2 * bs, tr_d + 3 * bs,  tr_d + 4 * bs, tr_d + 5 * bs,
                       tr_d + 6 * bs, tr_d + 8 * bs, tr_d + 10 * bs, tr_d + 12 * bs, tr_d + 15 * bs};
    u.part = part; u.acc = acc; u.nblk = wc.nblk; u.nrb = wc.nrb; u.samples = samples; u.warmup = warmup; u.wstride = wstride;
    u.burnIn = op->burnIn; u.kind = op->kind; u.taille = taille; u.npar = npar; u.params_move = params_move ? 1 : 0;
    u.fix_p0 = fixq[0] ? 1 : 0; u.fix_p1 = fixq[1] ? 1 : 0; u.fix_sigma = op->fix_sigma ? 1 : 0;
    u.parseval = 1.0 / ((double)M * N); u.dimX = (double)dimX; u.npix = (double)P;
    u.min_eta = log(op->min_th); u.max_eta = log(op->max_th); u.th_init = op->th_init;
    // d/d alpha of alpha^2 (1 + alpha^2 r^2 / beta)^(-(beta+2)/2) / (2 pi) carries alpha / pi; utils/diff_moffat_alpha.m:17 (and
    // with it psf_taps.inc, which reproduces the reference for the TV family) has alpha / (2 pi): half the derivative, in every
    // tap and in the sum.  This entry has no reference run to reproduce and states G_p as the derivative of the data term
    // (tests/test_wavelet_sb_cpu.py checks it against a finite difference), so the factor is restored here, exactly.
    u.g0_scale = op->kind == SBTV_PSF_MOFFAT ? 2.0 : 1.0;
    u.c_p0 = op->c_p[0]; u.c_p1 = op->c_p[1]; u.c_sigma = op->c_sigma; u.p_min0 = op->p_min[0]; u.p_max0 = op->p_max[0];
    u.p_min1 = op->p_min[1]; u.p_max1 = op->p_max[1]; u.p_true0 = op->p_true[0]; u.p_true1 = op->p_true[1];
    u.s_lo = op->sigma2_min; u.s_hi = op->sigma2_max; u.sigma2_init = op->sigma2; u.phi = op->phi;

    // constants, chain state, start taps; spectra of the PSF (H, D1, D2) and of y; the start state
    const double eta_init = log(op->th_init);                                // :101
    std::vector<WavSbChain> ch((size_t)batch);
    {
        const bool b1 = op->burnIn == 1;
        for (int b = 0; b < batch; ++b) {
            const double p0 = pinit[2 * (size_t)b], p1 = pinit[2 * (size_t)b + 1];
            ch[b] = WavSbChain{eta_init, op->th_init, op->th_init, p0, p1, op->sigma2, b1 ? eta_init : 0.0, b1 ? p0 : 0.0,
                               b1 ? p1 : 0.0, b1 ? op->sigma2 : 0.0, b1 ? 1.0 : 0.0, {0.0, 0.0, 0.0, 0.0}, 0.0};
        }
        SBTV_HIP(ctx, hipMemcpyAsync(u.chain, ch.data(), sizeof(WavSbChain) * batch, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(u.par, par_h.data(), sizeof(double) * 3 * t2 * batch, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(tr_d, 0, sizeof(double) * trlen, ctx->stream));
    }
    const double *tp[3] = {u.par, u.par + t2 * batch, u.par + 2 * t2 * batch};
    double2 *up[3] = {wc.op.Hs, D1s, D2s};
    auto spectra = [&]() -> int { return psf_spectrum_sets(ctx, wc.op.fp, tp, taille, up, npar > 1 ? 3 : 2); };
    SBTV_TRY(spectra());
    SBTV_TRY(wav_chain_start(ctx, wc));
    // S = column spectrum of W X, then the row pass without store: ||B W X - y||^2 and <dB/dp_q W X, B W X - y> -> acc
    auto residual_pass = [&]() -> int {
        SBTV_TRY(wav_chain_spectrum(ctx, wc));
        return wav_chain_rows(ctx, wc, OP_GRAD, acc, D1s, D2s);
    };
    auto update = [&](int phase, int ii, double delta) -> int {
        hipLaunchKernelGGL(wav_sb_update_kernel, dim3(batch), dim3(WAV_EWB), 0, ctx->stream, u, phase, ii, delta);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };
    // the start state: its spectrum for the first gradient pass, logpi(1) (:166)
    SBTV_TRY(residual_pass());
    SBTV_TRY(wav_abs_sum(ctx, wc, part));
    SBTV_TRY(update(WB_PH_START, 1, 0.0));
    ctx->calls += batch;
    // the lagging theta and sigma2(ii-1) of chain b, where the update kernel keeps them
    const WavStepPar sp{&u.chain->th_prev, &u.chain->sig2, (int)(sizeof(WavSbChain) / sizeof(double))};
    // MYULA step number `step` of the call (warm-up steps first, as the noise array is laid out) and its update
    auto iteration = [&](size_t step, int phase, int ii) -> int {
        SBTV_TRY(wav_chain_rows(ctx, wc, OP_GRADF, acc));                     // G from the column spectrum in S, with the current H
        const RngArgs r{op->seed, (unsigned)step, (unsigned)op->chain_offset, nullptr};
        SBTV_TRY(wav_chain_step(ctx, wc, sp, op->gamma, op->lambda, r, part));
        SBTV_TRY(residual_pass());
        // delta(ii) of :111
        const double delta = phase == WB_PH_MAIN ? op->d_scale * (pow((double)ii, -op->d_exp) / (double)dimX) : 0.0;
        SBTV_TRY(update(phase, ii, delta));
        if (phase == WB_PH_MAIN && params_move) SBTV_TRY(spectra());
        ctx->calls += 2 * (long long)batch;
        return 0;
    };
    for (int ii = 2; ii <= warmup; ++ii) {                                   // :131-141
        SBTV_TRY(iteration((size_t)(ii - 2), WB_PH_WARMUP, ii));
        if ((ii & 1023) == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int ii = 2; ii <= samples; ++ii) {                                  // :171-216
        SBTV_TRY(iteration((size_t)wsteps + (size_t)(ii - 2), WB_PH_MAIN, ii));
        if ((ii & 1023) == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }

    std::vector<double> tr(trlen);
    SBTV_HIP(ctx, hipMemcpyAsync(tr.data(), tr_d, sizeof(double) * trlen, hipMemcpyDeviceToHost, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(ch.data(), u.chain, sizeof(WavSbChain) * batch, hipMemcpyDeviceToHost, ctx->stream));
    SBTV_TRY(stage_out_copy(ctx, xw_last, X, ccnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int nmean = samples - op->burnIn;
    const double *t_th = tr.data(), *t_s = t_th + bs, *t_gx = t_th + 2 * bs, *t_lp = t_th + 3 * bs, *t_tol = t_th + 4 * bs,
                 *t_mean = t_th + 5 * bs, *t_ps = t_th + 6 * bs, *t_tolp = t_th + 8 * bs, *t_meanp = t_th + 10 * bs,
                 *t_gr = t_th + 12 * bs, *t_wu = t_th + 15 * bs;
    for (int b = 0; b < batch; ++b) {
        const size_t o = (size_t)b * samples;
        for (int q = 0; q < 4; ++q) eb[(size_t)b * 4 + q] = ch[b].eb[q];
        for (int i = 0; i < samples; ++i) {
            // slot 0 is the start value: theta(1), p(:, 1), sigma2(1)  (:146,151)
            if (thetas) thetas[o + i] = i ? t_th[o + i] : op->th_init;
            if (sigmas) sigmas[o + i] = i ? t_s[o + i] : op->sigma2;
            if (gx) gx[o + i] = t_gx[o + i];
            if (logpi) logpi[o + i] = t_lp[o + i];
            if (tol_thetas) tol_thetas[o + i] = t_tol[o + i];
            for (int q = 0; q < 2; ++q) {
                if (ps) ps[2 * o + (size_t)q * samples + i] = i ? t_ps[2 * o + (size_t)q * samples + i] : pinit[2 * (size_t)b + q];
                if (tol_ps) tol_ps[2 * o + (size_t)q * samples + i] = t_tolp[2 * o + (size_t)q * samples + i];
            }
            for (int q = 0; grads && q < 3; ++q) grads[3 * o + (size_t)q * samples + i] = t_gr[3 * o + (size_t)q * samples + i];
        }
        for (int i = 0; i < nmean; ++i) {
            if (mean_thetas) mean_thetas[(size_t)b * nmean + i] = t_mean[o + i];
            for (int q = 0; mean_ps && q < 2; ++q)
                mean_ps[((size_t)b * 2 + q) * nmean + i] = t_meanp[2 * o + (size_t)q * samples + i];
        }
        for (int i = 0; logpi_wu && i < warmup; ++i) logpi_wu[(size_t)b * warmup + i] = t_wu[(size_t)b * wstride + i];
    }
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

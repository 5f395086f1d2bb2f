// SAPG estimation of theta, the PSF parameters and sigma2 on the TV model with SK-ROCK as its Markov kernel:
// the loop of sbtv_SAPG_algorithm (sapg.hip) with its MYULA move replaced by one step of sbtv_skrock (skrock.hip).
// include/sbtv.h states the algorithm.  Nothing of either is copied: the arithmetic of the parameter step is sapg_step.inc, the
// per-chain update kernel sapg_chain_update.inc (shared with sapg_masked.hip), the stage kernels and the stepper that drives
// them skrock_stage.inc, and the refusals, the constants, the start state, the device set-up and the copy-out of the traces are
// the sapg_* functions of sampler_common.hip, shared with sapg.hip and sapg_masked.hip.
//
// One step on the context's stream: the spectra of the taps the previous update left in `par` (a free PSF parameter only),
// `stages` x (cold Chambolle prox, op_gradf on the stage's input, one stage kernel), one gradient-sum pass on the new sample
// (forward column pass with the TV partials where fft_cols_tv_ok allows, row pass OP_GRAD without store or inverse) and
// sapg_chain_update_kernel (sapg_chain_update.inc), one workgroup per chain: it totals the chain's sums, steps its parameters, books its traces and
// builds the taps of the new PSF parameters.  The stage kernels read sigma2 and lambda theta from the device, so nothing in
// a step waits for the host: one synchronisation per 1024 steps and one at the end.
#include <cmath>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

#include "sapg_step.inc"

namespace {

#include "skrock_stage.inc"          // SkrockStepper and its kernels
#include "sapg_chain_update.inc"     // SapgChainDev, sapg_chain_update_kernel
constexpr int SAPG_SK_SYNC = 1024;     // steps between two synchronisations

inline bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_SAPG_skrock(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const sbtv_sapg_opts *op,
                     const sbtv_sapg_skrock_step *sk, const double *x0, const double *noise, double *thetas, double *ps,
                     double *sigmas, double *logpi, double *logpi_wu, double *gx, double *grads, double *eb, double *x_last,
                     const sbtv_moments_opts *mo, double *post_mean, double *post_var, long long *post_count, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(sapg_refuse(ctx, "SAPG_skrock", y, M, N, batch, op));   // what sbtv_SAPG_algorithm refuses, with its codes
    // ---- its own
    if (op->share_gradients) return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: share_gradients is not offered");
    if (!sk) return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: the step (stages, dt, eta) is required");
    if (sk->stages < 2) return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: need stages >= 2");
    if (!positive_finite(sk->dt) || !positive_finite(sk->eta))
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: dt and eta must be finite and > 0");
    const int samples = op->samples, warmup = op->warmup, stages = sk->stages, chambolleit = op->chambolleit;
    const bool dev = (flags & SBTV_DEVICE_PTRS) != 0;
    // the moments request: the checks of sbtv_skrock, first = 0 meaning burnIn.  The chains estimate their own parameters, so
    // two of them never sample one posterior
    MomReq sel{};
    const MomReq *selp = nullptr;
    SBTV_TRY(mom_resolve(ctx, "SAPG_skrock", mo, op->burnIn, samples, post_mean, post_var, post_count, dev, &sel, &selp));
    if (selp && sel.pooled && batch > 1)
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: pooled = 1 needs chains of one posterior");

    // ---- the constants of the parameter step, the chains' start, the taps and derivative taps of p_init (the host's)
    SapgChainDev u{};
    sapg_fill_const(&u, op, M, N, batch, false, 1.0 / ((double)M * N));
    const bool params_move = u.params_move != 0;
    const size_t P = (size_t)M * N, cnt = P * batch;
    std::vector<SapgChain> chain;
    std::vector<double> hp, tr;
    SBTV_TRY(sapg_start(ctx, "SAPG_skrock", u, op, &chain, &hp));

    // ---- buffers
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    BlurOp bop;
    SBTV_TRY(op_open(ctx, "sapgsk", M, N, batch, "Y", &bop));
    ProxPlan pp;
    SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
    const bool tv_fused = fft_cols_tv_ok(bop.fp);
    const int nrb = fft_rows_blocks(bop.fp);
    const double *yd = nullptr, *x0d = nullptr;
    SBTV_TRY(stage_in(ctx, "sapgsk.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "sapgsk.grad", x0, cnt, flags, &x0d));            // staged where the gradient goes later
    double *A = nullptr, *K = nullptr, *prox = nullptr, *grad = nullptr, *Z = nullptr, *acc_g = nullptr, *acc = nullptr,
           *tvc = nullptr, *pm_mean = nullptr, *pm_m2 = nullptr;
    double2 *D1s = nullptr, *D2s = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "sapgstp.X", x_last, cnt, flags, &A));
    SBTV_TRY(ws_get_t(ctx, "sapgsk.K", cnt, &K));                            // the second image buffer
    SBTV_TRY(ws_get_t(ctx, "sapgsk.prox", cnt, &prox));
    SBTV_TRY(ws_get_t(ctx, "sapgsk.grad", cnt, &grad));
    if (noise && !dev) SBTV_TRY(ws_get_t(ctx, "sapgsk.Z", cnt, &Z));
    SBTV_TRY(ws_get_t(ctx, "sapgsk.D1", bop.fp.u_img * batch, &D1s));
    // a one-parameter PSF (Laplace) has one derivative spectrum: the second one the row pass reads IS the first
    if (u.npar > 1) SBTV_TRY(ws_get_t(ctx, "sapgsk.D2", bop.fp.u_img * batch, &D2s));
    else D2s = D1s;
    const size_t accn = (size_t)batch * 3 * nrb;
    SBTV_TRY(ws_get_t(ctx, "sapgsk.accg", accn, &acc_g));                    // residual sums of the stages' passes: not used
    SBTV_TRY(ws_get_t(ctx, "sapgsk.acc", accn, &acc));
    const int ntvc = tv_fused ? fft_cols_blocks(bop.fp) : 0;
    if (tv_fused) SBTV_TRY(ws_get_t(ctx, "sapgsk.tvc", (size_t)batch * ntvc, &tvc));
    if (selp) {
        SBTV_TRY(ws_get_t(ctx, "sapgsk.pm_mean", cnt, &pm_mean));
        SBTV_TRY(ws_get_t(ctx, "sapgsk.pm_m2", cnt, &pm_m2));
    }
    SapgDevBufs d{};
    SBTV_TRY(sapg_device_setup(ctx, "sapgsk", u, op, chain, hp, &d));
    double *par = d.par, *lam_d = par + 3 * (size_t)u.taille * u.taille * batch, *sig_d = lam_d + batch;
    u.acc = acc; u.tvp = tvc; u.nrb = nrb; u.ntv = ntvc; u.pctrl = pp.ctrl;
    u.scal = d.scal; u.chain = d.chain; u.par = par; u.delta = d.delta; u.traces = d.traces;
    auto spectra = [&] { return sapg_spectra(ctx, bop.fp, u, par, bop.Hs, D1s, D2s); };
    SBTV_TRY(spectra());
    SBTV_TRY(op_spectrum(ctx, bop.fp, yd, nullptr, bop.S, bop.Ys));
    // X = x0, or y  (SAPG_algorithm_Guassian.m:10-12)
    const double *start = x0d ? x0d : yd;
    if (start != A) SBTV_HIP(ctx, hipMemcpyAsync(A, start, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, nullptr));
    const ProxArm arm{pp.ctrl, lam_d, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, nullptr};

    // X <- SKROCK_step(X) at the parameters on the device: the sample sits in stp.X.  Steps count from 0 through the warm-up
    SkrockStepper stp{ctx, &bop, &pp, arm, NoiseFeed{ctx, noise, Z, cnt}, A, K, prox, grad, acc_g, sig_d, pm_mean, pm_m2,
                     op->lambda, P, batch, stages, chambolleit, op->seed, (unsigned)op->chain_offset};
    SBTV_TRY(stp.table(sk->eta, sk->dt));
    const unsigned steps = (unsigned)((warmup > 0 ? warmup - 1 : 0) + samples - 1);
    // momk > 0: the new sample is sample momk of the moments
    auto skrock_step = [&](int momk) -> int {
        SBTV_TRY(stp.step(momk, stp.done + 1u < steps));
        if (stp.done % SAPG_SK_SYNC == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return 0;
    };
    // ||A X - y||^2, <dA/dp_q X, A X - y> and TVnorm(X) of the sample with the current spectra, then the update kernel
    auto sums_and_update = [&](int phase, int ii) -> int {
        RowsArgs a{};
        a.dir_fwd = 1;
        a.op = OP_GRAD;
        a.H = bop.Hs;
        a.Y = bop.Ys;
        a.D1 = D1s;
        a.D2 = D2s;
        a.acc = acc;
        if (!tv_fused) {                                                     // arbitrary-size path
            double *tvp = nullptr;
            SBTV_TRY(tvnorm_partials(ctx, stp.X, M, N, batch, &tvp, &u.ntv));
            u.tvp = tvp;
        }
        SBTV_TRY(fft_cols_fwd_f(ctx, bop.fp, stp.X, nullptr, bop.S, nullptr, tvc));
        SBTV_TRY(fft_rows(ctx, bop.fp, bop.S, nullptr, a));
        hipLaunchKernelGGL(sapg_chain_update_kernel, dim3(batch), dim3(SAPG_CHAIN_WG), 0, ctx->stream, u, phase, ii);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };

    // ---- warm-up (:66-93) at th_init, p_init, sigma2_init, then logpi(1) and sample 1 of the moments
    for (int ii = 2; ii <= warmup; ++ii) {
        SBTV_TRY(skrock_step(0));
        SBTV_TRY(sums_and_update(SAPG_CHAIN_WARMUP, ii));
    }
    SBTV_TRY(sums_and_update(SAPG_CHAIN_START, 1));
    if (mom_sample_of(selp, 1)) SBTV_TRY(moments_seed(ctx, stp.X, pm_mean, pm_m2, P, batch));
    // ---- SAPG iterations (:98-248)
    for (int ii = 2; ii <= samples; ++ii) {
        if (params_move && ii > 2) SBTV_TRY(spectra());                      // of the taps the update of ii - 1 left in par
        SBTV_TRY(skrock_step(mom_sample_of(selp, ii)));
        SBTV_TRY(sums_and_update(SAPG_CHAIN_MAIN, ii));
    }

    // ---- the traces, the chains, the last sample and the moments -> the caller's arrays
    if (selp) SBTV_TRY(moments_finish(ctx, pm_mean, pm_m2, P, batch, mom_count(sel, samples), sel));
    SBTV_TRY(sapg_download(ctx, u, d, &tr, &chain));
    // the last sample sits in the caller's buffer or in the second one, as the parity of stages x steps has it
    if (dev && x_last && stp.X != x_last)
        SBTV_HIP(ctx, hipMemcpyAsync(x_last, stp.X, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(stage_out_copy(ctx, x_last, stp.X, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sapg_copy_out(u, op, tr.data(), chain.data(), nullptr, SapgOut{thetas, ps, sigmas, logpi, logpi_wu, gx, grads, eb});
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

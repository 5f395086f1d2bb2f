// MYULA sampling and SAPG estimation of theta, the PSF parameters and sigma2 on the TV model with a masked observation
// (DESIGN.md §3.16): the loops of sbtv_myula and sbtv_SAPG_algorithm (sapg.hip) on the likelihood
//     p(y | x, p, s2) ~ s2^(-n_obs/2) exp(-R / (2 s2)),   R = sum(m .* (B_p x - y).^2)
// include/sbtv.h states the model.  A mask breaks Parseval, so the middle of the gradient B'(m .* (Bx - y)) and the three
// parameter sums are spatial: one element-wise kernel forms the masked residual and leaves the partial sums, one kernel per
// chain totals them and runs the parameter step.  The arithmetic of that step is sapg_step.inc and its kernel
// sapg_chain_update.inc (shared with sapg_skrock.hip: `nobs` puts the observed pixels in place of dimX), the transforms are the
// row / column passes of the blur-operator layer, the prox is prox_iterate and the move is myula_step; the loop of
// sbtv_myula_masked is myula_plain_loop, and the refusals, the constants, the start state, the device set-up and the copy-out
// of sbtv_SAPG_masked are the sapg_* functions of sampler_common.hip: all shared with the circular drivers, not copied.
//
// One SAPG iteration on the context's stream: the MYULA move with the gradient and the prox the previous iteration left, the
// cold Chambolle prox of the new sample, one forward column pass of it (with the TV partials where fft_cols_tv_ok allows),
// B X, dB/dp_1 X and dB/dp_2 X from that one column spectrum (three row passes OP_MUL_H, three inverse column passes; Laplace:
// two), the residual kernel with the derivative sums (the traces book G_p whether or not p is free, as sbtv_SAPG_algorithm's
// do), the update kernel, then
//   PSF fixed:  B' r from the r the residual kernel wrote (forward column pass, row pass OP_MUL_HC, inverse column pass): no
//               spectrum is rebuilt;
//   PSF free:   the spectra of the new taps, B X again from the column spectrum still held (X has not moved), the residual
//               kernel without the sums, and B' r.
// The warm-up and sbtv_myula_masked need no derivative sums: B X, the residual kernel without them, B' r.
// Nothing in an iteration waits for the host: one synchronisation per 1024 iterations and one at the end.
#include <cmath>
#include <cstring>
#include <vector>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

#include "sapg_step.inc"

namespace {

#include "sapg_chain_update.inc"     // SapgChainDev, sapg_chain_update_kernel
constexpr int MSB = WAV_EWB;           // lanes per workgroup of the kernels below (wav_block_sum sums four waves)
constexpr int SAPG_MK_SYNC = 1024;     // iterations between two synchronisations

// r = m .* (Bx - y) over the pairs of chain blockIdx.y, written over Bx, and the partial sums of this workgroup in
// acc[chain][3][gridDim.x]: R = sum(m .* (Bx - y).^2) and, with DER, <D1x, r> and <D2x, r> (without: zeros).  A pixel with
// m = 0 gives r = 0 whatever y holds there.  16 bytes per lane and array; the sums run over the lane's pairs in order, then
// through the fixed tree of wav_block_sum: no atomics, so a chain's sums do not depend on the batch it runs in.
template <bool DER>
__global__ __launch_bounds__(MSB) void masked_resid_kernel(double *__restrict__ br, const double *__restrict__ y,
                                                            const double *__restrict__ m, const double *__restrict__ d1,
                                                            const double *__restrict__ d2, double *__restrict__ acc, size_t P) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * P;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (size_t q = (size_t)blockIdx.x * MSB + threadIdx.x; q < P / 2; q += (size_t)gridDim.x * MSB) {
        const size_t o = base + 2 * q;
        const double2 bv = *reinterpret_cast<const double2 *>(br + o);
        const double2 yv = *reinterpret_cast<const double2 *>(y + o);
        const double2 mv = *reinterpret_cast<const double2 *>(m + o);
        const double dx = bv.x - yv.x, dy = bv.y - yv.y;
        double2 r;
        r.x = mv.x > 0.0 ? mv.x * dx : 0.0;
        r.y = mv.y > 0.0 ? mv.y * dy : 0.0;
        s0 += mv.x > 0.0 ? r.x * dx : 0.0;
        s0 += mv.y > 0.0 ? r.y * dy : 0.0;
        if (DER) {
            const double2 e1 = *reinterpret_cast<const double2 *>(d1 + o);
            const double2 e2 = *reinterpret_cast<const double2 *>(d2 + o);
            s1 += e1.x * r.x;
            s1 += e1.y * r.y;
            s2 += e2.x * r.x;
            s2 += e2.y * r.y;
        }
        *reinterpret_cast<double2 *>(br + o) = r;
    }
    const double t0 = wav_block_sum(s0, red);
    const double t1 = DER ? wav_block_sum(s1, red) : 0.0;
    const double t2 = DER ? wav_block_sum(s2, red) : 0.0;
    if (threadIdx.x == 0) {
        const size_t G = gridDim.x;
        acc[((size_t)b * 3 + 0) * G + blockIdx.x] = t0;
        acc[((size_t)b * 3 + 1) * G + blockIdx.x] = t1;
        acc[((size_t)b * 3 + 2) * G + blockIdx.x] = t2;
    }
}

// partial counts of the pixels of chain blockIdx.y with m > 0 in nobs[chain][gridDim.x], once per call; reduce_partials
// totals them (sums of small integers: exact in any order)
__global__ __launch_bounds__(MSB) void masked_count_kernel(const double *__restrict__ m, double *__restrict__ nobs, size_t P) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * MSB + threadIdx.x; i < P; i += (size_t)gridDim.x * MSB)
        s += m[(size_t)b * P + i] > 0.0 ? 1.0 : 0.0;
    const double t = wav_block_sum(s, red);
    if (threadIdx.x == 0) nobs[(size_t)b * gridDim.x + blockIdx.x] = t;
}

// with host pointers: every entry finite and >= 0, and a positive one in every chain
int check_mask_host(sbtv_ctx *ctx, const char *who, const double *mask, size_t P, int batch) {
    for (int b = 0; b < batch; ++b) {
        bool any = false;
        for (size_t i = 0; i < P; ++i) {
            const double v = mask[(size_t)b * P + i];
            if (!(v >= 0.0) || std::isinf(v))
                return fail(ctx, SBTV_ERR_BADARG, std::string(who) + ": the mask must be finite and non-negative");
            any = any || v > 0.0;
        }
        if (!any) return fail(ctx, SBTV_ERR_BADARG, std::string(who) + ": a chain's mask observes no pixel");
    }
    return 0;
}

// The masked likelihood of one call on the blur-operator layer: S holds the column spectrum of the image fwd() was given
// last, S2 is the work spectrum of every transform that must leave S alone.
struct MaskedOp {
    sbtv_ctx *ctx;
    BlurOp bop;
    double2 *S2;
    const double *yd, *md;
    double *R, *acc;           // B x, then r = m .* (B x - y) in its place; the residual kernel's partial sums [batch][3][nblk]
    int nblk;

    // out = real(ifft2(U .* fft2(x))) from the column spectrum in S
    int through(const double2 *U, double *out) const {
        RowsArgs a{};
        a.dir_fwd = a.dir_inv = 1;
        a.op = OP_MUL_H;
        a.H = U;
        SBTV_TRY(fft_rows(ctx, bop.fp, bop.S, S2, a));
        return fft_cols_inv(ctx, bop.fp, S2, out, bop.inv_scale);
    }
    // r and R from the column spectrum in S with the current H; d1x / d2x non-null: also the two derivative sums
    int residual(const double *d1x, const double *d2x) const {
        SBTV_TRY(through(bop.Hs, R));
        const dim3 grid(nblk, bop.batch), block(MSB);
        if (d1x)
            hipLaunchKernelGGL(masked_resid_kernel<true>, grid, block, 0, ctx->stream, R, yd, md, d1x, d2x, acc, bop.P);
        else
            hipLaunchKernelGGL(masked_resid_kernel<false>, grid, block, 0, ctx->stream, R, yd, md, (const double *)nullptr,
                               (const double *)nullptr, acc, bop.P);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    }
    // grad = B' r (the gradient of the likelihood times sigma2); S keeps the column spectrum of x
    int gradient(double *grad) const {
        RowsArgs a{};
        a.dir_fwd = a.dir_inv = 1;
        a.op = OP_MUL_HC;
        a.H = bop.Hs;
        SBTV_TRY(fft_cols_fwd(ctx, bop.fp, R, nullptr, S2));
        SBTV_TRY(fft_rows(ctx, bop.fp, S2, S2, a));
        return fft_cols_inv(ctx, bop.fp, S2, grad, bop.inv_scale);
    }
};

// plan, spectra workspaces, y and the mask on the device, the residual buffer and its partial sums
int masked_open(sbtv_ctx *ctx, const char *prefix, const double *y, const double *mask, int M, int N, int batch, int flags,
                MaskedOp *mk) {
    const std::string p = std::string(prefix) + ".";
    mk->ctx = ctx;
    SBTV_TRY(op_open(ctx, prefix, M, N, batch, nullptr, &mk->bop));
    const size_t cnt = mk->bop.P * batch;
    SBTV_TRY(ws_get_t(ctx, (p + "S2").c_str(), (size_t)batch * mk->bop.fp.s_img, &mk->S2));
    SBTV_TRY(stage_in(ctx, (p + "y").c_str(), y, cnt, flags, &mk->yd));
    SBTV_TRY(stage_in(ctx, (p + "mask").c_str(), mask, cnt, flags, &mk->md));
    SBTV_TRY(ws_get_t(ctx, (p + "R").c_str(), cnt, &mk->R));
    mk->nblk = ew_blocks(mk->bop.P);
    SBTV_TRY(ws_get_t(ctx, (p + "acc").c_str(), (size_t)batch * 3 * mk->nblk, &mk->acc));
    return 0;
}

// the chains of a call have their own masks (and in SAPG their own parameters), so their moments are never pooled
int masked_pooled(sbtv_ctx *ctx, const char *who, const MomReq *selp, int batch) {
    if (selp && selp->pooled && batch > 1) return fail(ctx, SBTV_ERR_BADARG, std::string(who) + ": pooled = 1 needs batch = 1");
    return 0;
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_myula_masked(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch, const double *taps,
                      int taille, double lambda, double gamma, const double *theta, const double *sigma2, int samples,
                      int chambolleit, unsigned long long seed, int chain_offset, const double *noise, double *x_out,
                      const sbtv_moments_opts *mo, double *post_mean, double *post_var, long long *post_count, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    // ---- what sbtv_myula refuses, with its codes
    if (!y || !taps || !theta || !sigma2 || !x_out || batch < 1 || samples < 2 || !(lambda > 0.0) || !(gamma > 0.0) ||
        chain_offset < 0)
        return fail(ctx, SBTV_ERR_BADARG, "myula_masked: bad arguments");
    if (chambolleit <= 0) return fail(ctx, SBTV_ERR_MAXITER, "myula_masked: chambolleit must be positive");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    SBTV_TRY(check_even_pixels(ctx, M, N));
    // ---- its own
    if (!mask) return fail(ctx, SBTV_ERR_BADARG, "myula_masked: the mask is missing");
    const bool dev = (flags & SBTV_DEVICE_PTRS) != 0;
    const size_t P = (size_t)M * N, cnt = P * batch;
    if (!dev) SBTV_TRY(check_mask_host(ctx, "myula_masked", mask, P, batch));
    MomReq sel{};
    const MomReq *selp = nullptr;
    const int last = samples > 2 ? samples - 1 : 1;
    SBTV_TRY(mom_resolve(ctx, "myula_masked", mo, 1, last, post_mean, post_var, post_count, dev, &sel, &selp));
    SBTV_TRY(masked_pooled(ctx, "myula_masked", selp, batch));

    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    MaskedOp mk;
    SBTV_TRY(masked_open(ctx, "myulam", y, mask, M, N, batch, flags, &mk));
    ProxPlan pp;
    SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
    double *X = nullptr, *prox = nullptr, *grad = nullptr, *Z = nullptr, *par = nullptr, *pm_mean = nullptr, *pm_m2 = nullptr;
    if (selp) {
        SBTV_TRY(ws_get_t(ctx, "myulam.pm_mean", cnt, &pm_mean));
        SBTV_TRY(ws_get_t(ctx, "myulam.pm_m2", cnt, &pm_m2));
    }
    SBTV_TRY(stage_out_buf(ctx, "myulam.X", x_out, cnt, flags, &X));
    SBTV_TRY(ws_get_t(ctx, "myulam.prox", cnt, &prox));
    SBTV_TRY(ws_get_t(ctx, "myulam.grad", cnt, &grad));
    if (noise && !dev) SBTV_TRY(ws_get_t(ctx, "myulam.Z", cnt, &Z));
    const size_t t2 = (size_t)taille * taille, npar = t2 * batch + 2 * (size_t)batch;
    SBTV_TRY(ws_get_t(ctx, "myulam.par", npar, &par));      // [taps | lambda*theta | sigma2]
    double *lam_d = par + t2 * batch, *sig_d = lam_d + batch;
    {
        std::vector<double> hpar(npar);
        for (size_t q = 0; q < t2 * batch; ++q) hpar[q] = taps[q];
        for (int b = 0; b < batch; ++b) {
            hpar[t2 * batch + b] = lambda * theta[b];           // proxG(x, lambda, theta)   (run_deblur_tv.m:126)
            hpar[t2 * batch + batch + b] = sigma2[b];
        }
        SBTV_HIP(ctx, hipMemcpyAsync(par, hpar.data(), sizeof(double) * npar, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));                    // the staging vector goes out of scope
    }
    SBTV_TRY(psf_spectrum(ctx, mk.bop.fp, par, taille, mk.bop.Hs));
    SBTV_HIP(ctx, hipMemcpyAsync(X, mk.yd, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));   // x = op.y  (:3,11)
    if (mom_sample_of(selp, 1)) SBTV_TRY(moments_seed(ctx, X, pm_mean, pm_m2, P, batch));                // iteration 1 = y
    SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, nullptr));
    const ProxArm arm{pp.ctrl, lam_d, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, nullptr};
    // the loop (:13-16): gradF = B'(m .* (B x - y)) / sigma2; one synchronisation per SAPG_MK_SYNC iterations
    const MyulaLoop loop{X, prox, grad, sig_d, &pp, arm, NoiseFeed{ctx, noise, Z, cnt}, gamma, lambda, P, batch, samples,
                         chambolleit, seed, chain_offset, selp, pm_mean, pm_m2, SAPG_MK_SYNC};
    SBTV_TRY(myula_plain_loop(ctx, loop, [&]() -> int {
        SBTV_TRY(fft_cols_fwd(ctx, mk.bop.fp, X, nullptr, mk.bop.S));
        SBTV_TRY(mk.residual(nullptr, nullptr));
        return mk.gradient(grad);
    }));
    if (selp) SBTV_TRY(moments_finish(ctx, pm_mean, pm_m2, P, batch, mom_count(sel, last), sel));
    SBTV_TRY(stage_out_copy(ctx, x_out, X, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

int sbtv_SAPG_masked(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch, const sbtv_sapg_opts *op,
                     const double *x0, const double *noise, double *thetas, double *ps, double *sigmas, double *logpi,
                     double *logpi_wu, double *gx, double *grads, double *eb, double *x_last, const sbtv_moments_opts *mo,
                     double *post_mean, double *post_var, long long *post_count, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(sapg_refuse(ctx, "SAPG_masked", y, M, N, batch, op));   // what sbtv_SAPG_algorithm refuses, with its codes
    // ---- its own
    if (!mask) return fail(ctx, SBTV_ERR_BADARG, "SAPG_masked: the mask is missing");
    if (op->share_gradients) return fail(ctx, SBTV_ERR_BADARG, "SAPG_masked: share_gradients is not offered");
    const bool dev = (flags & SBTV_DEVICE_PTRS) != 0;
    const size_t P = (size_t)M * N, cnt = P * batch;
    if (!dev) SBTV_TRY(check_mask_host(ctx, "SAPG_masked", mask, P, batch));
    const int samples = op->samples, warmup = op->warmup, chambolleit = op->chambolleit;
    MomReq sel{};
    const MomReq *selp = nullptr;
    SBTV_TRY(mom_resolve(ctx, "SAPG_masked", mo, op->burnIn, samples, post_mean, post_var, post_count, dev, &sel, &selp));
    SBTV_TRY(masked_pooled(ctx, "SAPG_masked", selp, batch));

    // ---- the constants of the parameter step (the sums are spatial: no Parseval factor), the chains' start, the taps and
    // derivative taps of p_init (the host's)
    SapgChainDev u{};
    sapg_fill_const(&u, op, M, N, batch, false, 1.0);
    const bool params_move = u.params_move != 0;
    std::vector<SapgChain> chain;
    std::vector<double> hp, tr;
    SBTV_TRY(sapg_start(ctx, "SAPG_masked", u, op, &chain, &hp));

    // ---- buffers
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    MaskedOp mk;
    SBTV_TRY(masked_open(ctx, "sapgm", y, mask, M, N, batch, flags, &mk));
    const FftPlan &fp = mk.bop.fp;
    ProxPlan pp;
    SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
    const bool tv_fused = fft_cols_tv_ok(fp);
    const double *x0d = nullptr;
    SBTV_TRY(stage_in(ctx, "sapgm.grad", x0, cnt, flags, &x0d));             // staged where the gradient goes later
    double *X = nullptr, *prox = nullptr, *grad = nullptr, *Z = nullptr, *D1x = nullptr, *D2x = nullptr, *tvc = nullptr,
           *nobs = nullptr, *pm_mean = nullptr, *pm_m2 = nullptr;
    double2 *D1s = nullptr, *D2s = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "sapgm.X", x_last, cnt, flags, &X));
    SBTV_TRY(ws_get_t(ctx, "sapgm.prox", cnt, &prox));
    SBTV_TRY(ws_get_t(ctx, "sapgm.grad", cnt, &grad));
    if (noise && !dev) SBTV_TRY(ws_get_t(ctx, "sapgm.Z", cnt, &Z));
    SBTV_TRY(ws_get_t(ctx, "sapgm.D1", fp.u_img * batch, &D1s));
    // a one-parameter PSF (Laplace) has one derivative: the second spectrum and the second image the kernels read ARE the first
    if (u.npar > 1) SBTV_TRY(ws_get_t(ctx, "sapgm.D2", fp.u_img * batch, &D2s));
    else D2s = D1s;
    SBTV_TRY(ws_get_t(ctx, "sapgm.D1x", cnt, &D1x));
    if (u.npar > 1) SBTV_TRY(ws_get_t(ctx, "sapgm.D2x", cnt, &D2x));
    else D2x = D1x;
    const int ntvc = tv_fused ? fft_cols_blocks(fp) : 0;
    if (tv_fused) SBTV_TRY(ws_get_t(ctx, "sapgm.tvc", (size_t)batch * ntvc, &tvc));
    if (selp) {
        SBTV_TRY(ws_get_t(ctx, "sapgm.pm_mean", cnt, &pm_mean));
        SBTV_TRY(ws_get_t(ctx, "sapgm.pm_m2", cnt, &pm_m2));
    }
    SBTV_TRY(ws_get_t(ctx, "sapgm.nobs", (size_t)batch * (mk.nblk + 1), &nobs));   // [batch] totals, then the partials
    SapgDevBufs d{};
    SBTV_TRY(sapg_device_setup(ctx, "sapgm", u, op, chain, hp, &d));
    double *par = d.par, *lam_d = par + 3 * (size_t)u.taille * u.taille * batch, *sig_d = lam_d + batch;
    u.acc = mk.acc; u.tvp = tvc; u.nrb = mk.nblk; u.ntv = ntvc; u.nobs = nobs;
    u.scal = d.scal; u.chain = d.chain; u.par = par; u.delta = d.delta; u.traces = d.traces;
    hipLaunchKernelGGL(masked_count_kernel, dim3(mk.nblk, batch), dim3(MSB), 0, ctx->stream, mk.md, nobs + batch, P);
    SBTV_HIP(ctx, hipGetLastError());
    SBTV_TRY(reduce_partials(ctx, nobs + batch, batch, mk.nblk, nobs));
    auto spectra = [&] { return sapg_spectra(ctx, fp, u, par, mk.bop.Hs, D1s, D2s); };
    SBTV_TRY(spectra());
    // X = x0, or y as given  (SAPG_algorithm_Guassian.m:10-12)
    const double *start = x0d ? x0d : mk.yd;
    if (start != X) SBTV_HIP(ctx, hipMemcpyAsync(X, start, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
    const ProxArm arm{pp.ctrl, lam_d, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, nullptr};
    const NoiseFeed nz{ctx, noise, Z, cnt};

    // R, TVnorm(X) and r of the sample with the current spectra; der: also <dB/dp_q X, r>
    auto sums = [&](bool der) -> int {
        if (!tv_fused) {                                                     // arbitrary-size path
            double *tvp = nullptr;
            SBTV_TRY(tvnorm_partials(ctx, X, M, N, batch, &tvp, &u.ntv));
            u.tvp = tvp;
        }
        SBTV_TRY(fft_cols_fwd_f(ctx, fp, X, nullptr, mk.bop.S, nullptr, tvc));
        if (der) {
            SBTV_TRY(mk.through(D1s, D1x));
            if (u.npar > 1) SBTV_TRY(mk.through(D2s, D2x));
        }
        return mk.residual(der ? D1x : nullptr, der ? D2x : nullptr);
    };
    auto update = [&](int phase, int ii) -> int {
        hipLaunchKernelGGL(sapg_chain_update_kernel, dim3(batch), dim3(SAPG_CHAIN_WG), 0, ctx->stream, u, phase, ii);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };
    unsigned step = 0;                                                       // steps count from 0 through the warm-up and on
    // X <- |X + gam (prox - X)/lamb - gam grad/sigma2 + sqrt(2 gam) Z| (:80-81,160-161) at the sigma2 on the device, then the
    // cold prox of the new sample at the lambda theta on the device (:82,162); momk > 0: sample momk of the moments
    auto move = [&](int momk) -> int {
        const double *zd = nullptr;
        SBTV_TRY(nz.get(step, &zd));
        const RngArgs r{op->seed, step, (unsigned)op->chain_offset, nullptr};
        const MomArgs ma{pm_mean, pm_m2, momk, nullptr, 1, 1};
        SBTV_TRY(myula_step(ctx, X, prox, grad, zd, sig_d, op->gamma, u.lamb, P, batch, &r, &arm, momk > 0 ? &ma : nullptr));
        SBTV_TRY(prox_iterate(ctx, pp, X, chambolleit, prox, true));
        if (++step % SAPG_MK_SYNC == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return 0;
    };

    // ---- the start: prox and gradient of X at th_init, p_init (:70, :134 form the same prox); warm-up (:66-93); logpi(1)
    SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, nullptr));
    SBTV_TRY(prox_iterate(ctx, pp, X, chambolleit, prox, true));
    SBTV_TRY(sums(false));
    SBTV_TRY(mk.gradient(grad));
    for (int ii = 2; ii <= warmup; ++ii) {
        SBTV_TRY(move(0));
        SBTV_TRY(sums(false));
        SBTV_TRY(update(SAPG_CHAIN_WARMUP, ii));
        SBTV_TRY(mk.gradient(grad));
    }
    SBTV_TRY(update(SAPG_CHAIN_START, 1));                                      // the sums of the state the loop starts from stand
    if (mom_sample_of(selp, 1)) SBTV_TRY(moments_seed(ctx, X, pm_mean, pm_m2, P, batch));
    // ---- SAPG iterations (:98-248)
    for (int ii = 2; ii <= samples; ++ii) {
        SBTV_TRY(move(mom_sample_of(selp, ii)));
        SBTV_TRY(sums(true));                                                // G_p is booked whether or not p is free
        SBTV_TRY(update(SAPG_CHAIN_MAIN, ii));
        if (ii == samples) break;
        if (params_move) {                                                   // r at p(ii): new spectra, B X from S (X has not moved)
            SBTV_TRY(spectra());
            SBTV_TRY(mk.residual(nullptr, nullptr));
        }
        SBTV_TRY(mk.gradient(grad));
    }

    // ---- the traces, the chains, the last sample and the moments -> the caller's arrays
    if (selp) SBTV_TRY(moments_finish(ctx, pm_mean, pm_m2, P, batch, mom_count(sel, samples), sel));
    SBTV_TRY(sapg_download(ctx, u, d, &tr, &chain));
    SBTV_TRY(stage_out_copy(ctx, x_last, X, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sapg_copy_out(u, op, tr.data(), chain.data(), nullptr, SapgOut{thetas, ps, sigmas, logpi, logpi_wu, gx, grads, eb});
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

// What the sampler drivers of the TV model share on the host (declared in sbtv_internal.h): the moments request and the
// "chains of one posterior" check of every entry that accumulates moments, the plain MYULA loop of sbtv_myula and
// sbtv_myula_masked, and the front and back end of the three SAPG drivers (sapg.hip, sapg_skrock.hip, sapg_masked.hip): the
// refusals, the constants of the parameter step, the start state, the device set-up and the copy-out of traces and EB means.
// No kernel lives here: the shared device code is sapg_step.inc, sapg_chain_update.inc, skrock_stage.inc and psf_taps.inc.
#include <cmath>
#include <cstring>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

#include "sapg_step.inc"

// ---- moments
int mom_resolve(sbtv_ctx *ctx, const char *who, const sbtv_moments_opts *mo, int first0, int last, double *mean, double *var,
                long long *count, bool dev, MomReq *sel, const MomReq **selp) {
    if (selp) *selp = nullptr;
    if (!mo && selp) {
        if (mean || var || count) return fail(ctx, SBTV_ERR_BADARG, std::string(who) + ": moment outputs without moments options");
        return 0;
    }
    if (!mo || !mean) return fail(ctx, SBTV_ERR_BADARG, std::string(who) + ": moments options and post_mean are required");
    const int first = mo->first == 0 ? first0 : mo->first;
    if (mo->thin < 1 || first < 1 || first > last)
        return fail(ctx, SBTV_ERR_BADARG, std::string(who) + ": need thin >= 1 and 1 <= first <= the last iteration");
    *sel = MomReq{first, mo->thin, mo->pooled ? 1 : 0, mean, var, count, dev, false};
    if (selp) *selp = sel;
    return 0;
}

int check_one_posterior(sbtv_ctx *ctx, const char *who, const double *y, size_t P, const double *taps, int taille,
                        const double *theta, const double *sigma2, int batch, bool dev) {
    const size_t t2 = (size_t)taille * taille;
    bool same = y && taps && theta && sigma2 && P > 0 && taille > 0;
    for (int b = 1; same && b < batch; ++b)
        same = theta[b] == theta[0] && sigma2[b] == sigma2[0] && !memcmp(taps, taps + b * t2, sizeof(double) * t2);
    if (same) {
        std::vector<double> yh;
        const double *yv = y;
        if (dev) {
            SBTV_HIP(ctx, hipSetDevice(ctx->device));
            yh.resize(P * batch);
            SBTV_HIP(ctx, hipMemcpy(yh.data(), y, sizeof(double) * P * batch, hipMemcpyDeviceToHost));
            yv = yh.data();
        }
        for (int b = 1; same && b < batch; ++b) same = !memcmp(yv, yv + b * P, sizeof(double) * P);
    }
    if (!same)
        return fail(ctx, SBTV_ERR_BADARG, std::string(who) + ": pooled = 1 needs chains with the same y, taps, theta and sigma2");
    return 0;
}

// ---- plain MYULA
int myula_plain_loop(sbtv_ctx *ctx, const MyulaLoop &a, const std::function<int()> &gradient) {
    for (int ii = 2; ii <= a.samples - 1; ++ii) {             // :13
        const size_t step = (size_t)(ii - 2);
        SBTV_TRY(prox_iterate(ctx, *a.pp, a.X, a.chambolleit, a.prox, true));                // :15
        SBTV_TRY(gradient());
        const double *zd = nullptr;
        SBTV_TRY(a.nz.get(step, &zd));
        const RngArgs r{a.seed, (unsigned)step, (unsigned)a.chain_offset, nullptr};
        const MomArgs ma{a.pm_mean, a.pm_m2, mom_sample_of(a.mom, ii), nullptr, 1, 1};
        SBTV_TRY(myula_plain_step(ctx, a.X, a.prox, a.grad, zd, a.sig_d, a.gamma, a.lambda, a.P, a.batch, &r, &a.arm,
                                  ma.k > 0 ? &ma : nullptr));                                       // :16
        if (a.sync_every > 0 && (ii - 1) % a.sync_every == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

// ---- SAPG: front end
int sapg_refuse(sbtv_ctx *ctx, const char *who, const double *y, int M, int N, int batch, const sbtv_sapg_opts *op) {
    const std::string w = std::string(who) + ": ";
    if (!y || !op || batch < 1) return fail(ctx, SBTV_ERR_BADARG, w + "bad arguments");
    if (op->kind < 0 || op->kind > 2) return fail(ctx, SBTV_ERR_PSF, w + "unknown PSF kind");
    SBTV_TRY(check_psf_fits(ctx, op->psf_size, M, N));
    if (op->samples < 2 || op->warmup < 0 || op->burnIn < 1 || op->burnIn > op->samples)
        return fail(ctx, SBTV_ERR_BADARG, w + "need samples >= 2, 1 <= burnIn <= samples");
    if (op->chambolleit <= 0) return fail(ctx, SBTV_ERR_MAXITER, w + "chambolleit must be positive");
    if (op->chain_offset < 0) return fail(ctx, SBTV_ERR_BADARG, w + "chain_offset must be >= 0");
    if (op->iter_offset < 0) return fail(ctx, SBTV_ERR_BADARG, w + "iter_offset must be >= 0");
    return check_even_pixels(ctx, M, N);
}

void sapg_fill_const(SapgConst *k, const sbtv_sapg_opts *op, int M, int N, int batch, bool shared, double parseval) {
    SapgConst &u = *k;
    const int warmup = op->warmup;
    u.kind = op->kind; u.taille = op->psf_size; u.npar = (op->kind == SBTV_PSF_LAPLACE) ? 1 : 2;
    u.nspec = shared ? 1 : batch;                // spectra sets (H, D1, D2, Y)
    u.batch = batch; u.shared = shared ? 1 : 0; u.samples = op->samples; u.warmup = warmup > 0 ? warmup : 1; u.burnIn = op->burnIn;
    u.params_move = !(op->fix_p[0] && (u.npar < 2 || op->fix_p[1])) ? 1 : 0;
    u.fix_p0 = op->fix_p[0]; u.fix_p1 = op->fix_p[1]; u.fix_sigma = op->fix_sigma;
    u.dimX = (double)M * N; u.parseval = parseval; u.lamb = op->lambda; u.c_theta = op->c_theta; u.c_p0 = op->c_p[0];
    u.c_p1 = op->c_p[1]; u.c_sigma = op->c_sigma; u.min_th = op->min_th; u.max_th = op->max_th; u.p_min0 = op->p_min[0];
    u.p_max0 = op->p_max[0]; u.p_min1 = op->p_min[1]; u.p_max1 = op->p_max[1]; u.p_true0 = op->p_true[0]; u.p_true1 = op->p_true[1];
    u.s_lo = fmin(op->sigma2_min, op->sigma2_max); u.s_hi = fmax(op->sigma2_min, op->sigma2_max);
    u.sigma2_init = op->sigma2_init; u.phi = op->phi; u.step_base = (double)(warmup > 0 ? warmup - 1 : 0);
}

SapgChain sapg_chain_start(const SapgConst &u, const sbtv_sapg_opts *op) {
    SapgChain c{op->th_init, op->p_init[0], u.npar > 1 ? op->p_init[1] : 0.0, op->sigma2_init, 0.0, 0.0, 0.0, 0.0};
    if (op->burnIn == 1) { c.sum_th = c.theta; c.sum_s = c.sig2; c.sum_p0 = c.p0; c.sum_p1 = c.p1; }
    return c;
}

int sapg_start(sbtv_ctx *ctx, const char *who, const SapgConst &u, const sbtv_sapg_opts *op, std::vector<SapgChain> *chain,
               std::vector<double> *par) {
    const SapgChain c0 = sapg_chain_start(u, op);
    const size_t batch = (size_t)u.batch, t2 = (size_t)u.taille * u.taille;
    chain->assign(batch, c0);
    std::vector<double> &hp = *par;
    hp.assign(3 * t2 * batch + 2 * batch, 0.0);
    const double pv[3] = {c0.p0, op->kind == SBTV_PSF_LAPLACE ? 0.0 : c0.p1, op->kind == SBTV_PSF_GAUSSIAN ? op->phi : 0.0};
    const int rc = sbtv_psf_taps(op->kind, u.taille, pv, hp.data(), hp.data() + t2 * batch, hp.data() + 2 * t2 * batch);
    if (rc != 0) return fail(ctx, rc, std::string(who) + ": PSF parameters out of range");
    for (size_t b = 1; b < batch; ++b)
        for (int s = 0; s < 3; ++s) memcpy(&hp[s * t2 * batch + b * t2], &hp[s * t2 * batch], sizeof(double) * t2);
    for (size_t b = 0; b < batch; ++b) {
        hp[3 * t2 * batch + b] = u.lamb * c0.theta;          // proxG(x, theta): 'lambda', op.lambda*theta  (run_Gaussian_demo.m:191)
        hp[3 * t2 * batch + batch + b] = c0.sig2;
    }
    return 0;
}

int sapg_device_setup(sbtv_ctx *ctx, const char *prefix, const SapgConst &u, const sbtv_sapg_opts *op,
                      const std::vector<SapgChain> &chain, const std::vector<double> &par, SapgDevBufs *d) {
    const std::string p = std::string(prefix) + ".";
    const size_t ntr = sapg_traces_len(u);
    SBTV_TRY(ws_get_t(ctx, (p + "par").c_str(), par.size(), &d->par));
    SBTV_TRY(ws_get_t(ctx, (p + "scal").c_str(), 4 * (size_t)u.batch, &d->scal));
    SBTV_TRY(ws_get_t(ctx, (p + "delta").c_str(), (size_t)u.samples + 1, &d->delta));
    SBTV_TRY(ws_get_t(ctx, (p + "chain").c_str(), (size_t)u.batch, &d->chain));
    SBTV_TRY(ws_get_t(ctx, (p + "traces").c_str(), ntr, &d->traces));
    std::vector<double> dl((size_t)u.samples + 1, 0.0);
    for (int ii = 2; ii <= u.samples; ++ii) dl[ii] = sapg_delta(op, u.dimX, ii);
    SBTV_HIP(ctx, hipMemcpyAsync(d->par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(d->delta, dl.data(), sizeof(double) * dl.size(), hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(d->chain, chain.data(), sizeof(SapgChain) * u.batch, hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(d->traces, 0, sizeof(double) * ntr, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));        // the staging vector goes out of scope
    return 0;
}

int sapg_spectra(sbtv_ctx *ctx, const FftPlan &fp, const SapgConst &u, const double *par, double2 *Hs, double2 *D1s,
                 double2 *D2s) {
    const size_t set = (size_t)u.taille * u.taille * u.nspec;
    const double *tp[3] = {par, par + set, par + 2 * set};
    double2 *up[3] = {Hs, D1s, D2s};
    return psf_spectrum_sets(ctx, fp, tp, u.taille, up, u.npar > 1 ? 3 : 2);
}

// ---- SAPG: back end
int sapg_download(sbtv_ctx *ctx, const SapgConst &u, const SapgDevBufs &d, std::vector<double> *tr,
                  std::vector<SapgChain> *chain) {
    tr->assign(sapg_traces_len(u), 0.0);
    SBTV_HIP(ctx, hipMemcpyAsync(tr->data(), d.traces, sizeof(double) * tr->size(), hipMemcpyDeviceToHost, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(chain->data(), d.chain, sizeof(SapgChain) * u.batch, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

void sapg_copy_out(const SapgConst &u, const sbtv_sapg_opts *op, const double *tr, const SapgChain *chain,
                   const double *logpi0, const SapgOut &out) {
    const int samples = u.samples, warmup = op->warmup;
    const SapgTraces h = sapg_traces(const_cast<double *>(tr), u);
    for (int b = 0; b < u.batch; ++b) {
        const size_t o = (size_t)b * samples;
        if (out.thetas) { memcpy(out.thetas + o, h.theta + o, sizeof(double) * samples); out.thetas[o] = op->th_init; }
        if (out.sigmas) { memcpy(out.sigmas + o, h.sigma + o, sizeof(double) * samples); out.sigmas[o] = op->sigma2_init; }
        if (out.logpi) {
            memcpy(out.logpi + o, h.logpi + o, sizeof(double) * samples);
            if (logpi0) out.logpi[o] = logpi0[b];
        }
        if (out.gx) memcpy(out.gx + o, h.gx + o, sizeof(double) * samples);
        if (out.ps) {
            memcpy(out.ps + 2 * o, h.p + 2 * o, sizeof(double) * 2 * samples);
            out.ps[2 * o] = op->p_init[0];
            out.ps[2 * o + samples] = u.npar > 1 ? op->p_init[1] : 0.0;
        }
        if (out.grads) memcpy(out.grads + 4 * o, h.grads + 4 * o, sizeof(double) * 4 * samples);
        if (out.logpi_wu && warmup > 0)
            memcpy(out.logpi_wu + (size_t)b * warmup, h.wu + (size_t)b * warmup, sizeof(double) * warmup);
        if (out.eb) {
            const double cntm = (double)(samples - op->burnIn + 1);
            out.eb[(size_t)b * 4 + 0] = chain[b].sum_th / cntm;
            out.eb[(size_t)b * 4 + 1] = chain[b].sum_p0 / cntm;
            out.eb[(size_t)b * 4 + 2] = chain[b].sum_p1 / cntm;
            out.eb[(size_t)b * 4 + 3] = chain[b].sum_s / cntm;
        }
    }
}

}  // namespace sbtv

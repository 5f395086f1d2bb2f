// SAPG estimation of theta, the PSF parameters and sigma2 on the TV model with SK-ROCK as its Markov kernel:
// the loop of sbtv_SAPG_algorithm (sapg.hip) with its MYULA move replaced by one step of sbtv_skrock (skrock.hip).
// include/sbtv.h states the algorithm.  The arithmetic of the parameter step is sapg_step.inc, the stage kernels are
// skrock_stage.inc: both are shared with those drivers, not copied.
//
// One step on the context's stream: the spectra of the taps the previous update left in `par` (a free PSF parameter only),
// `stages` x (cold Chambolle prox, op_gradf on the stage's input, one stage kernel), one gradient-sum pass on the new sample
// (forward column pass with the TV partials where fft_cols_tv_ok allows, row pass OP_GRAD without store or inverse) and
// sapg_skrock_update_kernel, one workgroup per chain: it totals the chain's sums, steps its parameters, books its traces and
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

#include "skrock_stage.inc"
constexpr int SAPG_SK_SYNC = 1024;     // steps between two synchronisations

struct SapgSkDev : SapgConst {
    const double *acc;         // [batch][3][nrb]: sums of the gradient-sum row pass, ||AX-y||^2 and the two <dA_p X, AX-y>
    const double *tvp;         // [batch][ntv]: partial sums of TVnorm(X)
    int nrb, ntv;
    double *scal;              // [4*batch]: the totals, in the layout sapg_gradients reads (sapg_collect_kernel's)
    SapgChain *chain;          // [batch]
    ProxCtrl *pctrl;           // [batch]: the control blocks the last stage kernel armed, with lambda theta(ii-1)
    double *par;               // [taps | d0 | d1] of every chain, lam[batch], sigma2[batch]
    const double *delta;       // [samples + 1]: delta(ii), tabulated by the host (pow)
    SapgTraces tr;             // device traces
};
// what the update kernel does with the sums: logpi_wu(ii) of warm-up iteration ii; logpi(1) of the state the SAPG loop starts
// from; the parameter step of SAPG iteration ii
enum { SAPG_SK_WARMUP = 0, SAPG_SK_START = 1, SAPG_SK_MAIN = 2 };

// Collector and parameter update of the MYULA loop (sapg_collect_kernel + sapg_update_kernel) as one launch, one workgroup
// per chain, so that chain b of a batch is computed exactly as alone.  The four sums are totalled in the order of
// skrock_trace_kernel; one lane then runs sapg_gradients / sapg_step; with a free PSF parameter the workgroup builds the
// taps and both derivative taps of p(ii), summed in MATLAB's column-major order by one lane per set as in sapg_update_kernel
// (one path for every mask size: 15 x 15 is 225 lanes).
__global__ __launch_bounds__(SKB) void sapg_skrock_update_kernel(SapgSkDev u, int phase, int ii) {
    __shared__ double red[4], sf[SKB], se0[SKB], se1[SKB], ssum[3], pnew[2];
    const int b = blockIdx.x, tid = threadIdx.x, t2 = u.taille * u.taille;
    double tot[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double *p = q < 3 ? u.acc + ((size_t)b * 3 + q) * u.nrb : u.tvp + (size_t)b * u.ntv;
        const int n = q < 3 ? u.nrb : u.ntv;
        double s = 0.0;
        for (int i = tid; i < n; i += SKB) s += p[i];
        tot[q] = wav_block_sum(s, red);
    }
    if (tid == 0) {
        for (int q = 0; q < 3; ++q) u.scal[(size_t)b * 3 + q] = tot[q];
        u.scal[3 * (size_t)u.batch + b] = tot[3];
        SapgChain c = u.chain[b];
        if (phase == SAPG_SK_WARMUP) {
            u.tr.wu[(size_t)b * u.warmup + (ii - 1)] = sapg_logpi(u, c, u.scal, b);                  // :85
        } else if (phase == SAPG_SK_START) {
            u.tr.logpi[(size_t)b * u.samples] = sapg_logpi(u, c, u.scal, b);                         // :131
        } else {
            double G[4];
            sapg_gradients(u, u.tr, c, u.scal, b, ii, G);
            sapg_step(u, u.tr, c, b, ii, u.delta[ii], G);
            u.chain[b] = c;
            double *lam_d = u.par + (size_t)3 * t2 * u.batch, *sig_d = lam_d + u.batch;
            lam_d[b] = u.lamb * c.theta;         // proxG(x, theta): 'lambda', op.lambda*theta  (run_Gaussian_demo.m:191)
            sig_d[b] = c.sig2;
            u.pctrl[b].lambda = lam_d[b];        // the first prox of the next step is already armed: it runs at theta(ii) too
            pnew[0] = c.p0;
            pnew[1] = c.p1;
        }
    }
    if (phase != SAPG_SK_MAIN || !u.params_move) return;
    __syncthreads();
    const double pv[3] = {pnew[0], u.kind == 2 ? 0.0 : pnew[1], u.kind == 0 ? u.phi : 0.0};
    double f = 0.0, e0 = 0.0, e1 = 0.0;
    if (tid < t2) psf_taps_point(u.kind, u.taille, pv, tid, &f, &e0, &e1);
    sf[tid] = f;
    se0[tid] = e0;
    se1[tid] = e1;
    __syncthreads();
    if (tid < 3) {
        const double *v = tid == 0 ? sf : (tid == 1 ? se0 : se1);
        double a = 0.0;                          // MATLAB sum(k(:)): column-major order
        for (int q = 0; q < t2; ++q) a += v[q];
        ssum[tid] = a;
    }
    __syncthreads();
    if (tid < t2) {
        const double a = ssum[0];
        const size_t set = (size_t)t2 * u.batch, o = (size_t)b * t2 + tid;
        u.par[o] = f / a;
        u.par[set + o] = (e0 * a - f * ssum[1]) / (a * a);
        u.par[2 * set + o] = (e1 * a - f * ssum[2]) / (a * a);
    }
}

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
    // ---- what sbtv_SAPG_algorithm refuses, with its codes
    if (!y || !op || batch < 1) return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: bad arguments");
    if (op->kind < 0 || op->kind > 2) return fail(ctx, SBTV_ERR_PSF, "SAPG_skrock: unknown PSF kind");
    const int taille = op->psf_size;
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    if (op->samples < 2 || op->warmup < 0 || op->burnIn < 1 || op->burnIn > op->samples)
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: need samples >= 2, 1 <= burnIn <= samples");
    if (op->chambolleit <= 0) return fail(ctx, SBTV_ERR_MAXITER, "SAPG_skrock: chambolleit must be positive");
    if (op->chain_offset < 0) return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: chain_offset must be >= 0");
    if (op->iter_offset < 0) return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: iter_offset must be >= 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
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
    if (mo) {
        if (!post_mean) return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: moments options and post_mean are required");
        const int first = mo->first == 0 ? op->burnIn : mo->first;
        if (mo->thin < 1 || first < 1 || first > samples)
            return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: need thin >= 1 and 1 <= first <= samples");
        if (mo->pooled && batch > 1)
            return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: pooled = 1 needs chains of one posterior");
        sel = MomReq{first, mo->thin, mo->pooled ? 1 : 0, post_mean, post_var, post_count, dev, false};
        selp = &sel;
    } else if (post_mean || post_var || post_count) {
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_skrock: moment outputs without moments options");
    }

    // ---- the constants of the parameter step (those of sapg.hip)
    SapgSkDev u{};
    u.kind = op->kind; u.taille = taille; u.npar = (op->kind == SBTV_PSF_LAPLACE) ? 1 : 2; u.nspec = batch; u.batch = batch;
    u.shared = 0; u.samples = samples; u.warmup = warmup > 0 ? warmup : 1; u.burnIn = op->burnIn;
    const bool params_move = !(op->fix_p[0] && (u.npar < 2 || op->fix_p[1]));
    u.params_move = params_move ? 1 : 0; u.fix_p0 = op->fix_p[0]; u.fix_p1 = op->fix_p[1]; u.fix_sigma = op->fix_sigma;
    u.dimX = (double)M * N; u.parseval = 1.0 / ((double)M * N); u.lamb = op->lambda; u.c_theta = op->c_theta; u.c_p0 = op->c_p[0];
    u.c_p1 = op->c_p[1]; u.c_sigma = op->c_sigma; u.min_th = op->min_th; u.max_th = op->max_th; u.p_min0 = op->p_min[0];
    u.p_max0 = op->p_max[0]; u.p_min1 = op->p_min[1]; u.p_max1 = op->p_max[1]; u.p_true0 = op->p_true[0]; u.p_true1 = op->p_true[1];
    u.s_lo = fmin(op->sigma2_min, op->sigma2_max); u.s_hi = fmax(op->sigma2_min, op->sigma2_max);
    u.sigma2_init = op->sigma2_init; u.phi = op->phi; u.step_base = (double)(warmup > 0 ? warmup - 1 : 0);
    const size_t P = (size_t)M * N, cnt = P * batch, t2 = (size_t)taille * taille;
    const size_t npar = 3 * t2 * batch + 2 * (size_t)batch;

    // the chains' start, and the taps and derivative taps of p_init (the host's, as in sbtv_SAPG_algorithm)
    SapgChain c0{op->th_init, op->p_init[0], u.npar > 1 ? op->p_init[1] : 0.0, op->sigma2_init, 0.0, 0.0, 0.0, 0.0};
    if (op->burnIn == 1) { c0.sum_th = c0.theta; c0.sum_s = c0.sig2; c0.sum_p0 = c0.p0; c0.sum_p1 = c0.p1; }
    std::vector<SapgChain> chain(batch, c0);
    std::vector<double> hp(npar);
    {
        const double pv[3] = {c0.p0, op->kind == SBTV_PSF_LAPLACE ? 0.0 : c0.p1, op->kind == SBTV_PSF_GAUSSIAN ? op->phi : 0.0};
        const int rc = sbtv_psf_taps(op->kind, taille, pv, hp.data(), hp.data() + t2 * batch, hp.data() + 2 * t2 * batch);
        if (rc != 0) return fail(ctx, rc, "SAPG_skrock: PSF parameters out of range");
        for (int b = 1; b < batch; ++b)
            for (int s = 0; s < 3; ++s) memcpy(&hp[s * t2 * batch + b * t2], &hp[s * t2 * batch], sizeof(double) * t2);
        for (int b = 0; b < batch; ++b) {
            hp[3 * t2 * batch + b] = u.lamb * c0.theta;      // proxG(x, theta): 'lambda', op.lambda*theta  (run_Gaussian_demo.m:191)
            hp[3 * t2 * batch + batch + b] = c0.sig2;
        }
    }
    // the coefficient table and the scalars of the stages
    std::vector<double> mu(stages), nu(stages), kappa(stages);
    SBTV_TRY(sbtv_skrock_coefficients(stages, sk->eta, mu.data(), nu.data(), kappa.data(), nullptr, nullptr));
    const double lambda = op->lambda, dt = sk->dt, q = sqrt(2 * dt), nu1q = nu[0] * q;
    std::vector<SkrockStage> st(stages);
    st[0] = SkrockStage{mu[0] * dt, 0.0, kappa[0] * q, nu1q};
    for (int j = 1; j < stages; ++j) st[j] = SkrockStage{mu[j] * dt, nu[j], kappa[j], nu1q};

    // ---- buffers
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    BlurOp bop;
    SBTV_TRY(op_open(ctx, "sapgsk", M, N, batch, "Y", &bop));
    ProxPlan pp;
    SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
    const bool tv_fused = fft_cols_tv_ok(bop.fp), noise_host = noise && !dev;
    const int nrb = fft_rows_blocks(bop.fp), nblk = ew_blocks(P);
    const double *yd = nullptr, *x0d = nullptr;
    SBTV_TRY(stage_in(ctx, "sapgsk.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "sapgsk.grad", x0, cnt, flags, &x0d));            // staged where the gradient goes later
    double *A = nullptr, *K = nullptr, *prox = nullptr, *grad = nullptr, *Z = nullptr, *par = nullptr, *acc_g = nullptr,
           *acc = nullptr, *tvc = nullptr, *scal = nullptr, *delta_d = nullptr, *tr_d = nullptr, *pm_mean = nullptr,
           *pm_m2 = nullptr;
    double2 *D1s = nullptr, *D2s = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "sapgsk.X", x_last, cnt, flags, &A));
    SBTV_TRY(ws_get_t(ctx, "sapgsk.K", cnt, &K));                            // the second image buffer
    SBTV_TRY(ws_get_t(ctx, "sapgsk.prox", cnt, &prox));
    SBTV_TRY(ws_get_t(ctx, "sapgsk.grad", cnt, &grad));
    if (noise_host) SBTV_TRY(ws_get_t(ctx, "sapgsk.Z", cnt, &Z));
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
    SBTV_TRY(ws_get_t(ctx, "sapgsk.par", npar, &par));
    SBTV_TRY(ws_get_t(ctx, "sapgsk.scal", 4 * (size_t)batch, &scal));
    SBTV_TRY(ws_get_t(ctx, "sapgsk.delta", (size_t)samples + 1, &delta_d));
    SBTV_TRY(ws_get_t(ctx, "sapgsk.chain", (size_t)batch, &u.chain));
    std::vector<double> tr(sapg_traces_len(u), 0.0);
    SBTV_TRY(ws_get_t(ctx, "sapgsk.traces", tr.size(), &tr_d));
    double *lam_d = par + 3 * t2 * batch, *sig_d = lam_d + batch;
    u.acc = acc; u.tvp = tvc; u.nrb = nrb; u.ntv = ntvc; u.scal = scal; u.pctrl = pp.ctrl; u.par = par; u.delta = delta_d;
    u.tr = sapg_traces(tr_d, u);
    {
        std::vector<double> dl((size_t)samples + 1, 0.0);
        for (int ii = 2; ii <= samples; ++ii) dl[ii] = sapg_delta(op, u.dimX, ii);
        SBTV_HIP(ctx, hipMemcpyAsync(par, hp.data(), sizeof(double) * npar, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(delta_d, dl.data(), sizeof(double) * dl.size(), hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(u.chain, chain.data(), sizeof(SapgChain) * batch, hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(tr_d, 0, sizeof(double) * tr.size(), ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));                    // the staging vector goes out of scope
    }
    // spectra of the taps and of their parameter derivatives in `par`, ONE launch for the two or three sets
    auto spectra = [&]() -> int {
        const double *tp[3] = {par, par + t2 * batch, par + 2 * t2 * batch};
        double2 *up[3] = {bop.Hs, D1s, D2s};
        return psf_spectrum_sets(ctx, bop.fp, tp, taille, up, u.npar > 1 ? 3 : 2);
    };
    SBTV_TRY(spectra());
    SBTV_TRY(op_spectrum(ctx, bop.fp, yd, nullptr, bop.S, bop.Ys));
    // X = x0, or y  (SAPG_algorithm_Guassian.m:10-12)
    const double *start = x0d ? x0d : yd;
    if (start != A) SBTV_HIP(ctx, hipMemcpyAsync(A, start, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, nullptr));
    const ProxArm arm{pp.ctrl, lam_d, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, nullptr};

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
    // one stage: the drift at U (prox and gradient with the current H), then the stage kernel
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
    unsigned step = 0;                                                       // steps count from 0 through the warm-up and on
    const unsigned steps = (unsigned)((warmup > 0 ? warmup - 1 : 0) + samples - 1);
    // X <- SKROCK_step(X) at the parameters on the device; momk > 0: the new sample is sample momk of the moments
    auto skrock_step = [&](int momk) -> int {
        const RngArgs r{op->seed, step, (unsigned)op->chain_offset, nullptr};
        const bool more = step + 1u < steps;
        if (step == 0) {
            SBTV_TRY(stage_noise(0));
            hipLaunchKernelGGL(skrock_perturb_kernel, grid, block, 0, ctx->stream, (const double *)X, Pb, normals(0), nu1q, P, r,
                               arm);
            SBTV_HIP(ctx, hipGetLastError());
        }
        double *U = Pb, *V = X;                                              // K_{j-1} (stage 1: P), K_{j-2}
        SBTV_TRY(stage(U, V, 1, false, r, nullptr));
        if (more) SBTV_TRY(stage_noise(step + 1u));                          // after FIRST, before LAST
        for (int j = 2; j <= stages; ++j) {
            const MomArgs mc{pm_mean, pm_m2, j == stages ? momk : 0, nullptr, 1, 1};
            SBTV_TRY(stage(U, V, j, more, r, &mc));
            std::swap(U, V);                                                 // U = K_j, V = K_{j-1} (after the last: P_next)
        }
        X = U;
        Pb = V;
        if (++step % SAPG_SK_SYNC == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
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
            SBTV_TRY(tvnorm_partials(ctx, X, M, N, batch, &tvp, &u.ntv));
            u.tvp = tvp;
        }
        SBTV_TRY(fft_cols_fwd_f(ctx, bop.fp, X, nullptr, bop.S, nullptr, tvc));
        SBTV_TRY(fft_rows(ctx, bop.fp, bop.S, nullptr, a));
        hipLaunchKernelGGL(sapg_skrock_update_kernel, dim3(batch), dim3(SKB), 0, ctx->stream, u, phase, ii);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };

    // ---- warm-up (:66-93) at th_init, p_init, sigma2_init, then logpi(1) and sample 1 of the moments
    for (int ii = 2; ii <= warmup; ++ii) {
        SBTV_TRY(skrock_step(0));
        SBTV_TRY(sums_and_update(SAPG_SK_WARMUP, ii));
    }
    SBTV_TRY(sums_and_update(SAPG_SK_START, 1));
    if (mom_sample_of(selp, 1)) SBTV_TRY(moments_seed(ctx, X, pm_mean, pm_m2, P, batch));
    // ---- SAPG iterations (:98-248)
    for (int ii = 2; ii <= samples; ++ii) {
        if (params_move && ii > 2) SBTV_TRY(spectra());                      // of the taps the update of ii - 1 left in par
        SBTV_TRY(skrock_step(mom_sample_of(selp, ii)));
        SBTV_TRY(sums_and_update(SAPG_SK_MAIN, ii));
    }

    // ---- the traces, the chains, the last sample and the moments -> the caller's arrays
    if (selp) SBTV_TRY(moments_finish(ctx, pm_mean, pm_m2, P, batch, mom_count(sel, samples), sel));
    SBTV_HIP(ctx, hipMemcpyAsync(tr.data(), tr_d, sizeof(double) * tr.size(), hipMemcpyDeviceToHost, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(chain.data(), u.chain, sizeof(SapgChain) * batch, hipMemcpyDeviceToHost, ctx->stream));
    // the last sample sits in the caller's buffer or in the second one, as the parity of stages x steps has it
    if (dev && x_last && X != x_last)
        SBTV_HIP(ctx, hipMemcpyAsync(x_last, X, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(stage_out_copy(ctx, x_last, X, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const SapgTraces h = sapg_traces(tr.data(), u);
    for (int b = 0; b < batch; ++b) {
        const size_t o = (size_t)b * samples;
        if (thetas) { memcpy(thetas + o, h.theta + o, sizeof(double) * samples); thetas[o] = op->th_init; }
        if (sigmas) { memcpy(sigmas + o, h.sigma + o, sizeof(double) * samples); sigmas[o] = op->sigma2_init; }
        if (logpi) memcpy(logpi + o, h.logpi + o, sizeof(double) * samples);
        if (gx) memcpy(gx + o, h.gx + o, sizeof(double) * samples);
        if (ps) {
            memcpy(ps + 2 * o, h.p + 2 * o, sizeof(double) * 2 * samples);
            ps[2 * o] = op->p_init[0];
            ps[2 * o + samples] = u.npar > 1 ? op->p_init[1] : 0.0;
        }
        if (grads) memcpy(grads + 4 * o, h.grads + 4 * o, sizeof(double) * 4 * samples);
        if (logpi_wu && warmup > 0) memcpy(logpi_wu + (size_t)b * warmup, h.wu + (size_t)b * warmup, sizeof(double) * warmup);
        if (eb) {
            const double cntm = (double)(samples - op->burnIn + 1);
            eb[(size_t)b * 4 + 0] = chain[b].sum_th / cntm;
            eb[(size_t)b * 4 + 1] = chain[b].sum_p0 / cntm;
            eb[(size_t)b * 4 + 2] = chain[b].sum_p1 / cntm;
            eb[(size_t)b * 4 + 3] = chain[b].sum_s / cntm;
        }
    }
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

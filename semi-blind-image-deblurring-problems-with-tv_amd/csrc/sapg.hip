// The plain MYULA chain (SALSA/myula.m) and the SAPG / MYULA parameter-estimation loop
// (SAPG/SAPG_algorithm_Guassian.m, _moffat.m, _laplace.m) as device-resident loops over the TV-prox and
// spectral-operator kernels.
#include <cmath>
#include <cstring>

#include "sbtv_internal.h"

namespace sbtv {

// SAPG scalars of one iteration in one launch: block (q, b) reduces, in a fixed order, the rows-kernel accumulator
// q < 3 of image b (||AX-y||^2 and the two <dA_p X, AX-y> sums, [batch][3][nrb]) or, for q = 3, the periodic-TV
// partials ([batch][ntv]) and writes the total where the host reads it: out[b*3 + q] resp. out[3*batch + b].
// `out` is the device view of pinned host memory, so no copy kernel follows.
// Blocks q >= 4 (deferred stop rule of the multi-buffer prox, device-resident loop): block 4 + s totals the error
// partials of Chambolle step s into out[4*batch + b*FSTRIDE + s]; the parameter-update kernel applies the rule.
__global__ __launch_bounds__(256) void sapg_collect_kernel(const double *__restrict__ acc, int nrb,
                                                           const double *__restrict__ tvp, int ntv,
                                                           double *__restrict__ out, int batch,
                                                           const double *__restrict__ ppart, int pnblk) {
    __shared__ double red[4];
    const int q = blockIdx.x, b = blockIdx.y;
    if (q >= 4) {
        if (threadIdx.x >= 64) return;
        const int st = q - 4;
        const double tot = mb_step_sum(ppart + ((size_t)b * FSTRIDE + st) * pnblk, pnblk, threadIdx.x);
        if (threadIdx.x == 0) out[4 * (size_t)batch + (size_t)b * FSTRIDE + st] = tot;
        return;
    }
    const double *p = (q < 3) ? acc + ((size_t)b * 3 + q) * nrb : tvp + (size_t)b * ntv;
    const int n = (q < 3) ? nrb : ntv;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += p[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[(q < 3) ? (size_t)b * 3 + q : 3 * (size_t)batch + b] = (red[0] + red[1]) + (red[2] + red[3]);
}

#include "sapg_step.inc"   // SapgChain, SapgConst, SapgTraces, sapg_logpi / sapg_gradients / sapg_step, sapg_delta

struct SapgDev : SapgConst {
    const double *scal;        // [4*batch] totals of the collector: ||AX-y||^2, <dA_p0 X, r>, <dA_p1 X, r> per chain, TV
    SapgChain *chain;          // [batch]
    double *par;               // [taps | d0 | d1] per spectrum set, lam[batch], sigma2[batch], noise step
    const double *delta;       // [samples + 1]: delta(ii) of :55, tabulated by the host (pow)
    int *it;                   // [0] ii of the SAPG iteration in flight, [1] ii of the warm-up iteration in flight
    double *red;               // [6] shared-gradient sums (the all-reduce buffer)
    double *G;                 // [batch*4] per-chain gradients
    SapgTraces tr;             // device traces
    // deferred stop rule of the multi-buffer prox (null: the prox applies it itself): control blocks, the step sums the
    // collector left behind the scalars, and the launch geometry (prox_k steps, launch l ran prox_base + (l < prox_extra))
    ProxCtrl *pctrl;
    int prox_k, prox_base, prox_extra;
};
enum { SAPG_PH_GRADS = 1, SAPG_PH_UPDATE = 2, SAPG_PH_WARMUP = 4 };

__global__ __launch_bounds__(256) void sapg_update_kernel(SapgDev u, int phase) {
#pragma clang fp contract(off)
    __shared__ double sf[256], se0[256], se1[256], ssum[3];
    const int B = u.batch, tid = threadIdx.x, t2 = u.taille * u.taille;
    double *lam_d = u.par + (size_t)3 * t2 * u.nspec, *sig_d = lam_d + B, *step_d = sig_d + B;
    if (u.pctrl && (phase & (SAPG_PH_WARMUP | SAPG_PH_GRADS))) {
        // the stop rule of the prox this iteration ran optimistically (chambolle_prox_TV_stop.m:131): one thread per chain
        // books k / err and, if it stopped early, what the redo launch (which follows this kernel) has to repeat
        for (int b = tid; b < B; b += 256) {
            ProxCtrl c = u.pctrl[b];
            if (!c.done) {
                mb_apply_rule(c, u.scal + 4 * (size_t)B + (size_t)b * FSTRIDE, u.prox_k, u.prox_base, u.prox_extra);
                u.pctrl[b] = c;
            }
        }
    }
    if (phase & SAPG_PH_WARMUP) {
        // logPiTrace_WU(ii) of the warm-up iteration that just finished (:85); theta and sigma do not move here
        const int ii = u.it[1];
        for (int b = tid; b < B; b += 256) u.tr.wu[(size_t)b * u.warmup + (ii - 1)] = sapg_logpi(u, u.chain[b], u.scal, b);
        __syncthreads();
        if (tid == 0) {
            u.it[1] = ii + 1;
            *step_d = (double)(ii - 1);          // noise step of warm-up iteration ii+1 (steps count from 0 at ii = 2)
        }
        return;
    }
    const int ii = u.it[0];
    if (phase & SAPG_PH_GRADS) {
        for (int b = tid; b < B; b += 256) {
            const SapgChain c = u.chain[b];
            sapg_gradients(u, u.tr, c, u.scal, b, ii, u.G + b * 4);
        }
        __threadfence_block();
        __syncthreads();
        if (u.shared && tid == 0) {
            // the chains sample one posterior: G = mean over the chains (SAPG_algorithm_moffat.m:158-173), summed
            // here in chain order; the sums of the other ranks are added by the all-reduce between the two phases
            for (int q = 0; q < 4; ++q) {
                double a = 0;
                for (int b = 0; b < B; ++b) a += u.G[b * 4 + q];
                u.red[q] = a;
            }
            u.red[4] = (double)B;
            u.red[5] = 0.0;
        }
        __threadfence_block();
        __syncthreads();
    }
    if (!(phase & SAPG_PH_UPDATE)) return;
    // a rank whose iteration failed locally contributes {0, 0, 0, 0, 0 chains, 1}: the flag is latched (red[6] is outside
    // the six reduced doubles) and the host returns SBTV_ERR_PEER when it next looks at the device
    if (u.shared && tid == 0 && u.red[5] != 0.0) u.red[6] = 1.0;
    const double delta = u.delta[ii];
    for (int b = tid; b < B; b += 256) {
        SapgChain c = u.chain[b];
        double G[4];
        for (int q = 0; q < 4; ++q) G[q] = u.shared ? u.red[q] / u.red[4] : u.G[b * 4 + q];
        sapg_step(u, u.tr, c, b, ii, delta, G);
        u.chain[b] = c;
        lam_d[b] = u.lamb * c.theta;         // proxG(x, theta): 'lambda', op.lambda*theta  (run_Gaussian_demo.m:191)
        sig_d[b] = c.sig2;
    }
    __threadfence_block();
    __syncthreads();
    if (u.params_move && t2 <= 64) {
        // taps and derivative taps of the new PSF parameters (sbtv_psf_taps): one WAVE per spectrum set, four sets at a time
        // (a 7 x 7 mask is 49 lanes; the sums run over the taps in MATLAB's column-major order on lane 0, as below)
        const int w = tid >> 6, lane = tid & 63;
        for (int sset = w; sset < u.nspec; sset += 4) {
            const SapgChain c = u.chain[sset];
            const double pv[3] = {c.p0, u.kind == 2 ? 0.0 : c.p1, u.kind == 0 ? u.phi : 0.0};
            double f = 0.0, e0 = 0.0, e1 = 0.0;
            if (lane < t2) psf_taps_point(u.kind, u.taille, pv, lane, &f, &e0, &e1);
            sf[tid] = f;
            se0[tid] = e0;
            se1[tid] = e1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            double a = 0, a0 = 0, a1 = 0;
            if (lane == 0) {
                for (int q = 0; q < t2; ++q) {
                    a += sf[w * 64 + q];
                    a0 += se0[w * 64 + q];
                    a1 += se1[w * 64 + q];
                }
            }
            a = __shfl(a, 0, 64);
            a0 = __shfl(a0, 0, 64);
            a1 = __shfl(a1, 0, 64);
            if (lane < t2) {
                u.par[(size_t)sset * t2 + lane] = f / a;
                u.par[(size_t)t2 * u.nspec + (size_t)sset * t2 + lane] = (e0 * a - f * a0) / (a * a);
                u.par[(size_t)2 * t2 * u.nspec + (size_t)sset * t2 + lane] = (e1 * a - f * a1) / (a * a);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    } else if (u.params_move) {
        // masks above 8 x 8: one spectrum set after the other on the whole workgroup
        for (int sset = 0; sset < u.nspec; ++sset) {
            const SapgChain c = u.chain[sset];
            const double pv[3] = {c.p0, u.kind == 2 ? 0.0 : c.p1, u.kind == 0 ? u.phi : 0.0};
            psf_taps_block(u.kind, u.taille, pv, u.par, sset, u.nspec, sf, se0, se1, ssum);
            __syncthreads();
        }
    }
    if (tid == 0) {
        u.it[0] = ii + 1;
        *step_d = u.step_base + (double)(ii - 1);    // noise step of SAPG iteration ii+1
    }
}

}  // namespace sbtv

using namespace sbtv;

// ---------------------------------------------------------------------------
// a-6: plain MYULA chain at fixed parameters (SALSA/myula.m:1-22)
// ---------------------------------------------------------------------------
namespace sbtv {
static int myula_impl(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                      double lambda, double gamma, const double *theta, const double *sigma2, int samples, int chambolleit,
                      unsigned long long seed, int chain_offset, const double *noise, double *x_out, int flags,
                      const MomReq *mom) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!y || !taps || !theta || !sigma2 || !x_out || batch < 1 || samples < 2 || !(lambda > 0.0) || !(gamma > 0.0) ||
        chain_offset < 0)
        return fail(ctx, SBTV_ERR_BADARG, "myula: bad arguments");
    if (chambolleit <= 0) return fail(ctx, SBTV_ERR_MAXITER, "myula: chambolleit must be positive");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    SBTV_TRY(check_even_pixels(ctx, M, N));
    BlurOp bop;
    SBTV_TRY(op_open(ctx, "myula", M, N, batch, "Y", &bop));
    ProxPlan pp;
    SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
    const size_t P = bop.P, cnt = P * batch;
    const double *yd = nullptr;
    SBTV_TRY(stage_in(ctx, "myula.y", y, cnt, flags, &yd));
    const bool noise_host = noise && !(flags & SBTV_DEVICE_PTRS);
    double *X = nullptr, *prox = nullptr, *grad = nullptr, *Z = nullptr, *par = nullptr, *acc = nullptr;
    double *pm_mean = nullptr, *pm_m2 = nullptr;          // running mean / M2 of the samples [batch][P]
    if (mom) {
        SBTV_TRY(ws_get_t(ctx, "myula.pm_mean", cnt, &pm_mean));
        SBTV_TRY(ws_get_t(ctx, "myula.pm_m2", cnt, &pm_m2));
    }
    SBTV_TRY(stage_out_buf(ctx, "myula.X", x_out, cnt, flags, &X));
    SBTV_TRY(ws_get_t(ctx, "myula.prox", cnt, &prox));
    SBTV_TRY(ws_get_t(ctx, "myula.grad", cnt, &grad));
    if (noise_host) SBTV_TRY(ws_get_t(ctx, "myula.Z", cnt, &Z));
    SBTV_TRY(ws_get_t(ctx, "myula.acc", (size_t)batch * 3 * fft_rows_blocks(bop.fp), &acc));
    const size_t t2 = (size_t)taille * taille, npar = t2 * batch + 2 * (size_t)batch;
    SBTV_TRY(ws_get_t(ctx, "myula.par", npar, &par));      // [taps | lambda*theta | sigma2]
    double *taps_d = par, *lam_d = par + t2 * batch, *sig_d = lam_d + batch;
    std::vector<double> hpar(npar);
    for (size_t q = 0; q < t2 * batch; ++q) hpar[q] = taps[q];
    for (int b = 0; b < batch; ++b) {
        hpar[t2 * batch + b] = lambda * theta[b];           // proxG(x, lambda, theta)   (run_deblur_tv.m:126)
        hpar[t2 * batch + batch + b] = sigma2[b];
    }
    SBTV_HIP(ctx, hipMemcpyAsync(par, hpar.data(), sizeof(double) * npar, hipMemcpyHostToDevice, ctx->stream));
    SBTV_TRY(psf_spectrum(ctx, bop.fp, taps_d, taille, bop.Hs));
    SBTV_TRY(op_spectrum(ctx, bop.fp, yd, nullptr, bop.S, bop.Ys));
    SBTV_HIP(ctx, hipMemcpyAsync(X, yd, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));   // x = op.y  (:3,11)
    if (mom_sample_of(mom, 1)) SBTV_TRY(moments_seed(ctx, X, pm_mean, pm_m2, P, batch));            // iteration 1 = y
    SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, nullptr));
    const ProxArm arm{pp.ctrl, lam_d, chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, nullptr};
    // the loop (:13-16) never waits for the host; gradF = AT(A x - y) / sigma2   (run_deblur_tv.m:131)
    const MyulaLoop loop{X, prox, grad, sig_d, &pp, arm, NoiseFeed{ctx, noise, Z, cnt}, gamma, lambda, P, batch, samples,
                         chambolleit, seed, chain_offset, mom, pm_mean, pm_m2, 0};
    SBTV_TRY(myula_plain_loop(ctx, loop, [&] { return op_gradf(ctx, bop, X, acc, grad); }));
    if (mom) SBTV_TRY(moments_finish(ctx, pm_mean, pm_m2, P, batch, mom_count(*mom, samples > 2 ? samples - 1 : 1), *mom));
    SBTV_TRY(stage_out_copy(ctx, x_out, X, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}
}  // namespace sbtv

extern "C" {

int sbtv_myula(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille, double lambda,
               double gamma, const double *theta, const double *sigma2, int samples, int chambolleit,
               unsigned long long seed, int chain_offset, const double *noise, double *x_out, int flags) {
    return myula_impl(ctx, y, M, N, batch, taps, taille, lambda, gamma, theta, sigma2, samples, chambolleit, seed,
                      chain_offset, noise, x_out, flags, nullptr);
}

int sbtv_myula_moments(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                       double lambda, double gamma, const double *theta, const double *sigma2, int samples, int chambolleit,
                       unsigned long long seed, int chain_offset, const double *noise, double *x_out,
                       const sbtv_moments_opts *mo, double *post_mean, double *post_var, long long *post_count, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    MomReq mr;
    const bool dev = (flags & SBTV_DEVICE_PTRS) != 0;
    SBTV_TRY(mom_resolve(ctx, "myula_moments", mo, 1, samples > 2 ? samples - 1 : 1, post_mean, post_var, post_count, dev, &mr,
                         nullptr));
    if (mr.pooled && batch > 1)
        SBTV_TRY(check_one_posterior(ctx, "myula_moments", y, M > 0 && N > 0 ? (size_t)M * N : 0, taps, taille, theta, sigma2,
                                     batch, dev));
    return myula_impl(ctx, y, M, N, batch, taps, taille, lambda, gamma, theta, sigma2, samples, chambolleit, seed,
                      chain_offset, noise, x_out, flags, &mr);
}

// ---------------------------------------------------------------------------
// a-5 / a-6: SAPG with a MYULA kernel
// ---------------------------------------------------------------------------
int sbtv_SAPG_algorithm(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const sbtv_sapg_opts *op,
                        const double *x0, const double *noise, double *thetas, double *ps, double *sigmas,
                        double *logpi, double *logpi_wu, double *gx, double *grads, double *eb, double *x_last,
                        sbtv_allreduce_fn reduce_fn, void *reduce_user, int flags) {
    return sapg_impl(ctx, y, M, N, batch, op, x0, noise, thetas, ps, sigmas, logpi, logpi_wu, gx, grads, eb, x_last,
                     reduce_fn, reduce_user, flags, nullptr);
}

int sbtv_SAPG_algorithm_moments(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const sbtv_sapg_opts *op,
                                const double *x0, const double *noise, double *thetas, double *ps, double *sigmas,
                                double *logpi, double *logpi_wu, double *gx, double *grads, double *eb, double *x_last,
                                sbtv_allreduce_fn reduce_fn, void *reduce_user, const sbtv_moments_opts *mo,
                                double *post_mean, double *post_var, long long *post_count, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!op) return fail(ctx, SBTV_ERR_BADARG, "SAPG_algorithm_moments: bad arguments");
    MomReq mr;
    SBTV_TRY(mom_resolve(ctx, "SAPG_algorithm_moments", mo, op->burnIn, op->samples, post_mean, post_var, post_count,
                         (flags & SBTV_DEVICE_PTRS) != 0, &mr, nullptr));
    if (mr.pooled && !op->share_gradients && batch > 1)
        return fail(ctx, SBTV_ERR_BADARG, "SAPG_algorithm_moments: pooled = 1 needs chains of one posterior (share_gradients = 1)");
    return sapg_impl(ctx, y, M, N, batch, op, x0, noise, thetas, ps, sigmas, logpi, logpi_wu, gx, grads, eb, x_last,
                     reduce_fn, reduce_user, flags, &mr);
}

}  // extern "C"

namespace sbtv {

// One SAPG call on one stream: the arguments, the buffers, the pieces of an iteration and the two loops built from them.
// The iteration body (MYULA step, prox, operator pass, collector) exists once; the device-resident loop appends the
// update kernel(s) and never waits for the host, the host-side loop waits for the scalars and does the same arithmetic
// (sapg_gradients / sapg_step) itself.
struct SapgRun {
    // ---- the call (sapg_impl's arguments, in its order)
    sbtv_ctx *ctx; const double *y; int M, N, batch; const sbtv_sapg_opts *op; const double *x0, *noise;
    double *thetas, *ps, *sigmas, *logpi, *logpi_wu, *gx, *grads, *eb, *x_last;
    sbtv_allreduce_fn reduce_fn; void *reduce_user; int flags; const MomReq *mom;

    // ---- constants (u: the parameter step's, and in the device-resident loop the update kernel's arguments), buffers
    SapgDev u{};
    FftPlan fp, fps;
    ProxPlan pp;
    ProxArm arm{};
    size_t P = 0, cnt = 0, t2 = 0, npar_all = 0;
    int nrb = 0, ntvc = 0;
    double inv_scale = 0.0, gam = 0.0;
    bool noise_host = false, reduce_dev = false, dev_loop = false, fuse_myula = false, prox_mb = false, defer_rule = false,
         params_move = false;
    double *X = nullptr, *prox = nullptr, *grad = nullptr, *Z = nullptr, *acc = nullptr;
    double *pm_mean = nullptr, *pm_m2 = nullptr;          // running mean / M2 of the samples [batch][P]
    double2 *S = nullptr, *Hs = nullptr, *D1s = nullptr, *D2s = nullptr, *Ys = nullptr;
    double *par = nullptr;       // [taps | d0 | d1] per spectrum set, then lam[batch], sigma2[batch], noise step
    double *lam_d = nullptr, *sig_d = nullptr, *step_d = nullptr;
    double *tvc = nullptr;       // TV partials of X from the forward column pass [batch][fft_cols_blocks]
    double *scal_h = nullptr;    // pinned: the scalars of an iteration as the host sees them, then par_h
    double *par_h = nullptr;     // pinned staging for the per-iteration parameter upload, layout of par
    double *scal_d = nullptr;    // device-resident loop: the scalars of an iteration (+ the prox step sums)
    double *scal_out = nullptr;  // where the collector leaves the scalars: scal_d, or the device view of scal_h

    // ---- state
    std::vector<SapgChain> chain;             // the chains on the host (device-resident loop: the start, then the end state)
    std::vector<double> tr;                   // the traces on the host, layout of sapg_traces
    std::vector<double> logpi0;               // logPi of slot 0 (ii = 1)
    std::vector<double> last_p0, last_p1;     // the PSF parameters the taps in par_h were made from
    bool grad_in_S = false;      // S holds the spectrum of the gradient the next MYULA step needs
    size_t noise_step = 0;
    int main_ii = 0;             // the SAPG iteration being enqueued (0 in the warm-up): selects the moments' samples
    bool graphs_ok = false;      // hipGraph replay wanted and, so far, available
    GraphExecs graphs;
    bool collective_done = false, reduce_broken = false;      // in-stream collective of the iteration being enqueued

    bool in_stream() const { return u.shared && reduce_dev; }

    // spectra of the taps and of their parameter derivatives, ONE launch for the two or three sets
    int spectra() { return sapg_spectra(ctx, fps, u, par, Hs, D1s, D2s); }
    // taps / derivative taps of the chains' current PSF parameters, every spectrum set, into the pinned block
    int stage_taps() {
        for (int s = 0; s < u.nspec; ++s) {
            const SapgChain &c = chain[s];
            double pv[3] = {c.p0, (op->kind == SBTV_PSF_GAUSSIAN || op->kind == SBTV_PSF_MOFFAT) ? c.p1 : 0.0,
                            op->kind == SBTV_PSF_GAUSSIAN ? op->phi : 0.0};
            int rc = sbtv_psf_taps(op->kind, u.taille, pv, par_h + s * t2, par_h + t2 * u.nspec + s * t2,
                                   par_h + 2 * t2 * u.nspec + s * t2);
            if (rc != 0) return fail(ctx, rc, "SAPG_algorithm: PSF parameters out of range");
            last_p0[s] = c.p0;
            last_p1[s] = c.p1;
        }
        return 0;
    }
    // upload taps/derivative taps for the current parameters and rebuild the spectra (nothing to do if they did not move)
    int refresh_spectra() {
        bool dirty = false;
        for (int s = 0; s < u.nspec; ++s)
            if (!(chain[s].p0 == last_p0[s]) || !(chain[s].p1 == last_p1[s])) dirty = true;
        if (!dirty) return 0;
        SBTV_TRY(stage_taps());
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));     // par_h may still be in flight
        SBTV_HIP(ctx, hipMemcpyAsync(par, par_h, sizeof(double) * 3 * t2 * u.nspec, hipMemcpyHostToDevice, ctx->stream));
        return spectra();
    }
    // lambda*theta and sigma2 of the chains into the pinned block
    void stage_lam_sigma() {
        double *stage = par_h + 3 * t2 * u.nspec;
        for (int b = 0; b < batch; ++b) {
            stage[b] = u.lamb * chain[b].theta;       // proxG(x, theta): 'lambda', op.lambda*theta  (run_Gaussian_demo.m:191)
            stage[batch + b] = chain[b].sig2;
        }
    }
    int upload_lam_sigma() {
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        stage_lam_sigma();
        SBTV_HIP(ctx, hipMemcpyAsync(lam_d, par_h + 3 * t2 * u.nspec, sizeof(double) * 2 * batch, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    // The gradient's only reader is the MYULA step.  On the sizes of the wave-granular column pass its spectrum stays in S
    // and the inverse column pass that would store it runs as part of that step instead (fft_cols_inv_myula: no gradient
    // array, one launch less); SBTV_SAPG_FUSED_MYULA=0 or any other size: inverse pass here, element-wise step later.
    int gradient_from_S() {
        if (fuse_myula) {
            grad_in_S = true;
            return 0;
        }
        return fft_cols_inv(ctx, fp, S, grad, inv_scale);
    }
    // spectral pass over X with the CURRENT spectra: accumulates ||AX-y||^2 and <dA_q X, AX-y>, and (if want_grad)
    // leaves grad = AT(AX - y) (unscaled by sigma^2)
    int operator_pass(bool want_grad) {
        RowsArgs a{};
        a.dir_fwd = 1;
        a.dir_inv = want_grad ? 1 : 0;
        a.op = OP_GRAD;
        a.H = Hs;
        a.Y = Ys;
        a.D1 = D1s;
        a.D2 = D2s;
        a.acc = acc;
        a.shared_spec = u.shared;
        // TVnorm(X) (needed by the collector that follows every operator pass) rides on this column pass
        SBTV_TRY(fft_cols_fwd_f(ctx, fp, X, nullptr, S, nullptr, tvc));
        SBTV_TRY(fft_rows(ctx, fp, S, want_grad ? S : nullptr, a));
        if (want_grad) SBTV_TRY(gradient_from_S());
        return 0;
    }
    // spectra of the parameters moved by the previous iteration, then grad = AT(AX - y) with them.  The taps are already
    // in `par` when the parameters live on the device (device-resident loop, captured iteration); an eager iteration of
    // the host-side loop uploads them first, if they moved.
    int respec_gradient(bool in_graph) {
        SBTV_TRY((dev_loop || in_graph) ? spectra() : refresh_spectra());
        RowsArgs a{};
        a.dir_fwd = 1;
        a.dir_inv = 1;
        a.op = OP_GRADF;
        a.H = Hs;
        a.Y = Ys;
        a.acc = acc;
        a.shared_spec = u.shared;
        // S still holds colFFT(X): the gradient-sums pass that ended the previous iteration wrote no spectrum, and X
        // has not moved since - no second forward column pass
        SBTV_TRY(fft_rows(ctx, fp, S, S, a));
        return gradient_from_S();
    }
    // TVnorm(X) partials + ONE collector launch that reduces them together with the accumulators of the last
    // operator pass straight into pinned host memory (no separate reductions, no copy kernel)
    // steps > 0: the collector also totals the step sums of the prox just run (deferred stop rule)
    int collect_scalars(int steps) {
        double *tvp = tvc;
        int ntv = ntvc;
        if (!tvp) SBTV_TRY(tvnorm_partials(ctx, X, M, N, batch, &tvp, &ntv));      // arbitrary-size path
        hipLaunchKernelGGL(sapg_collect_kernel, dim3(4 + steps, batch), dim3(256), 0, ctx->stream, (const double *)acc, nrb,
                           (const double *)tvp, ntv, scal_out, batch, (const double *)pp.partials, pp.fnblk);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    }
    // until the host sees the scalars the collector has been asked for
    int wait_scalars() {
        if (dev_loop) SBTV_HIP(ctx, hipMemcpyAsync(scal_h, scal_d, sizeof(double) * 4 * batch, hipMemcpyDeviceToHost, ctx->stream));
        return wait_stream(ctx);
    }
    // X <- |X + gam (prox - X)/lamb - gam gradF + sqrt(2 gam) Z|  (:80-81,160-161).  With the device generator the
    // normals are drawn inside the step kernel (no Z array is written or read); injected noise goes through Z.
    // The step kernel also re-arms the prox control blocks for the cold-start prox that always follows it.
    // Posterior moments: the step of SAPG iteration main_ii (0 in the warm-up) also updates the running mean / M2 when
    // the iteration is selected; a captured iteration (in_graph) decides that on the device from u.it[0] == ii.
    int myula(bool in_graph) {
        const bool fused = grad_in_S;
        grad_in_S = false;
        MomArgs ma{pm_mean, pm_m2, 0, nullptr, mom ? mom->first : 1, mom ? mom->thin : 1};
        if (mom && main_ii > 0) {
            if (in_graph) ma.it = u.it;
            else ma.k = mom_sample_of(mom, main_ii);
        }
        const MomArgs *mp = (ma.k > 0 || ma.it) ? &ma : nullptr;
        if (noise) {
            SBTV_HIP(ctx, hipMemcpyAsync(Z, noise + noise_step * cnt, sizeof(double) * cnt,
                                         noise_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
            ++noise_step;
            if (fused) return fft_cols_inv_myula(ctx, fp, S, inv_scale, X, prox, Z, sig_d, gam, u.lamb, nullptr, &arm, mp);
            return myula_step(ctx, X, prox, grad, Z, sig_d, gam, u.lamb, P, batch, nullptr, &arm, mp);
        }
        const RngArgs r{op->seed, (unsigned)noise_step, (unsigned)op->chain_offset, in_graph ? step_d : nullptr};
        if (!in_graph) ++noise_step;
        if (fused) return fft_cols_inv_myula(ctx, fp, S, inv_scale, X, prox, nullptr, sig_d, gam, u.lamb, &r, &arm, mp);
        return myula_step(ctx, X, prox, grad, nullptr, sig_d, gam, u.lamb, P, batch, &r, &arm, mp);
    }
    // prox = chambolle(X, lambda*theta, cold start); armed: the MYULA step before it has reset the control blocks
    // Inside the device-resident loop the prox runs in the multi-buffer optimistic mode: its Chambolle launches go back to
    // back without stop-rule work in between (in-kernel or as separate kernels that costs 4-5 us per launch), every
    // launch boundary keeps its duals, one small kernel applies the rule over all steps and a (normally empty) redo
    // launch re-runs the steps up to an early stop.  Early stops DO happen here (small lambda*theta: err falls below
    // 1e-3 within the 25 iterations), so unlike SALSA / FISTA this path must handle them in place.
    // Deferred rule (default in the device-resident loop; SBTV_SAPG_DEFER=0: rule kernel + redo right after the launches):
    // the prox output is not needed before the NEXT iteration's MYULA step, so the step sums are totalled by blocks of
    // the collector, the rule is applied by the parameter-update kernel (both launched anyway) and only the (normally
    // empty) redo launch follows them - one launch of 7-8 us less per iteration.
    int do_prox(bool armed) {
        if (!armed) SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, op->chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, nullptr));
        return prox_iterate(ctx, pp, X, op->chambolleit, prox, true, (armed && prox_mb) ? (defer_rule ? 3 : 2) : 0);
    }

    // One iteration's device work up to its scalars; main = SAPG iteration (else warm-up), respec = new PSF spectra +
    // gradF first (`grad` already holds AT(AX-y) for the current spectra unless the PSF parameters moved at the end of
    // the previous iteration)
    int iteration_body(bool main, bool respec, bool in_graph) {
        if (respec) SBTV_TRY(respec_gradient(in_graph));
        SBTV_TRY(myula(in_graph));                                                             // :80-81 / :160-161
        SBTV_TRY(do_prox(true));                                                               // :82 / :162
        SBTV_TRY(operator_pass(main ? !params_move : true));                                   // G_w*, G_s, f  (:170-188)
        return collect_scalars(defer_rule ? op->chambolleit : 0);                              // incl. g(X)  (:165)
    }
    // hipGraph replay (small images: ~25 launches of a few microseconds per iteration make the loop launch-bound):
    // captures `body` into *exec the first time, then `stage`s the host side of this launch and replays.  *replayed stays
    // false when replay is not wanted or capture is unavailable; the caller then launches eagerly, now and from now on.
    template <class Body, class Stage>
    int replay(hipGraphExec_t *exec, bool *replayed, Body &&body, Stage &&stage) {
        *replayed = false;
        if (!graphs_ok) return 0;
        if (!*exec && (graph_begin(ctx) != 0 || graph_end(ctx, body(), exec) != 0)) {
            *exec = nullptr;
            graphs_ok = false;
            return 0;
        }
        SBTV_TRY(stage());
        SBTV_HIP(ctx, hipGraphLaunch(*exec, ctx->stream));
        *replayed = true;
        return 0;
    }

    int update(int phase) {
        hipLaunchKernelGGL(sapg_update_kernel, dim3(1), dim3(256), 0, ctx->stream, u, phase);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    }

    int setup() {
        // ---- the constants of the parameter step; one set of spectra (H, D1, D2, Y) for shared-gradient chains
        sapg_fill_const(&u, op, M, N, batch, op->share_gradients != 0, 1.0 / ((double)M * N));
        params_move = u.params_move != 0;
        SBTV_TRY(fft_plan(ctx, M, N, batch, &fp));
        SBTV_TRY(fft_plan(ctx, M, N, u.nspec, &fps));
        SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
        P = (size_t)M * N;
        cnt = P * batch;
        const int nspec = u.nspec;

        // ---- buffers
        const double *yd = nullptr, *x0d = nullptr;
        SBTV_TRY(stage_in(ctx, "sapg.y", y, u.shared ? P : cnt, flags, &yd));
        SBTV_TRY(stage_in(ctx, "sapg.x0", x0, cnt, flags, &x0d));
        noise_host = noise && !(flags & SBTV_DEVICE_PTRS);
        SBTV_TRY(ws_get_t(ctx, "sapg.X", cnt, &X));
        SBTV_TRY(ws_get_t(ctx, "sapg.prox", cnt, &prox));
        SBTV_TRY(ws_get_t(ctx, "sapg.grad", cnt, &grad));
        SBTV_TRY(ws_get_t(ctx, "sapg.Z", cnt, &Z));
        if (mom) {
            SBTV_TRY(ws_get_t(ctx, "sapg.pm_mean", cnt, &pm_mean));
            SBTV_TRY(ws_get_t(ctx, "sapg.pm_m2", cnt, &pm_m2));
        }
        const size_t spec = fp.u_img;
        SBTV_TRY(ws_get_t(ctx, "sapg.S", (size_t)batch * fp.s_img, &S));
        SBTV_TRY(ws_get_t(ctx, "sapg.H", spec * nspec, &Hs));
        SBTV_TRY(ws_get_t(ctx, "sapg.D1", spec * nspec, &D1s));
        // a one-parameter PSF (Laplace) has one derivative spectrum: the second one the gradient pass reads IS the first
        // (same memory: no third spectrum to compute, and its lines are already in the cache when the row pass asks again)
        if (u.npar > 1) SBTV_TRY(ws_get_t(ctx, "sapg.D2", spec * nspec, &D2s));
        else D2s = D1s;
        SBTV_TRY(ws_get_t(ctx, "sapg.Y", spec * nspec, &Ys));
        double2 *S1 = nullptr;
        SBTV_TRY(ws_get_t(ctx, "sapg.S1", (size_t)nspec * fp.s_img, &S1));
        t2 = (size_t)u.taille * u.taille;
        npar_all = 3 * t2 * nspec + 2 * (size_t)batch + 1;
        SBTV_TRY(ws_get_t(ctx, "sapg.par", npar_all, &par));
        lam_d = par + 3 * t2 * nspec;
        sig_d = lam_d + batch;
        step_d = sig_d + batch;
        nrb = fft_rows_blocks(fp);
        SBTV_TRY(ws_get_t(ctx, "sapg.acc", (size_t)batch * 3 * nrb, &acc));
        PinnedLayout lay;
        const auto f_scal = lay.add<double>(4 * (size_t)batch), f_par = lay.add<double>(npar_all);
        void *ph = nullptr, *pd = nullptr;
        SBTV_TRY(pinned_get(ctx, lay.bytes(), &ph, &pd));
        scal_h = f_scal.at(ph);
        scal_out = f_scal.at(pd);
        par_h = f_par.at(ph);
        ntvc = fft_cols_tv_ok(fp) ? fft_cols_blocks(fp) : 0;
        if (ntvc) SBTV_TRY(ws_get_t(ctx, "sapg.tvc", (size_t)batch * ntvc, &tvc));
        inv_scale = 1.0 / ((double)fp.n1 * N);
        gam = op->gamma;

        // ---- where the parameter updates run.  Default: on the device (sapg_update_kernel), the host only enqueues.
        // A host reduce_fn needs the gradients on the host every iteration, which selects the host-side loop.
        static const bool env_host_loop = [] {
            const char *e = getenv("SBTV_SAPG_HOST");
            return e && e[0] == '1';
        }();
        reduce_dev = reduce_fn && (flags & SBTV_REDUCE_DEVICE);
        dev_loop = !(flags & SBTV_SAPG_HOST_LOOP) && !env_host_loop && (!reduce_fn || reduce_dev);
        if (reduce_dev && !dev_loop)
            return fail(ctx, SBTV_ERR_BADARG, "SAPG_algorithm: SBTV_REDUCE_DEVICE needs the device-resident loop (no SBTV_SAPG_HOST_LOOP)");
        if (dev_loop) {
            SBTV_TRY(ws_get_t(ctx, "sapg.scal", (4 + (size_t)FSTRIDE) * batch, &scal_d));      // + the prox step sums
            scal_out = scal_d;
        }

        // ---- chain state, traces
        chain.assign(batch, sapg_chain_start(u, op));
        tr.assign(sapg_traces_len(u), 0.0);
        logpi0.assign(batch, 0.0);
        last_p0.assign(nspec, NAN);
        last_p1.assign(nspec, NAN);

        static const bool fuse_wanted = [] {
            const char *e = getenv("SBTV_SAPG_FUSED_MYULA");
            return !(e && e[0] == '0');
        }();
        fuse_myula = fuse_wanted && fft_cols_inv_step_ok(fp);
        arm = ProxArm{pp.ctrl, lam_d, op->chambolleit, CHAMBOLLE_TOL, CHAMBOLLE_TAU, nullptr};
        prox_mb = dev_loop && prox_spec_ok(pp, X, prox, op->chambolleit);
        if (prox_mb) SBTV_TRY(prox_reserve_pairs(ctx, &pp, prox_launches(pp, op->chambolleit) + 2));
        static const bool defer_wanted = [] {
            const char *e = getenv("SBTV_SAPG_DEFER");
            return !(e && e[0] == '0');
        }();
        defer_rule = prox_mb && defer_wanted;
        // Replay is opt-in.  The host-side loop has no device iteration counter to select the moments' samples from, and a
        // run with an in-stream collective has the collective enqueued by the caller's code: both launch eagerly.
        graphs_ok = (noise == nullptr) && graph_wanted(cnt) && !(mom && !dev_loop) && !in_stream();

        // ---- Y spectrum (one per spectrum set)
        SBTV_TRY(op_spectrum(ctx, fps, yd, nullptr, S1, Ys));
        // X0 = y by default (SAPG_algorithm_Guassian.m:10-12)
        if (x0d) {
            SBTV_HIP(ctx, hipMemcpyAsync(X, x0d, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            for (int b = 0; b < batch; ++b)
                SBTV_HIP(ctx, hipMemcpyAsync(X + (size_t)b * P, yd + (u.shared ? 0 : (size_t)b * P), sizeof(double) * P,
                                             hipMemcpyDeviceToDevice, ctx->stream));
        }
        return 0;
    }

    // The warm-up (:66-93) with `iteration(ii)` for ii = 2..warmup, then slot 0 of the traces (ii = 1): the one place where
    // the device-resident loop looks at the scalars
    template <class Iteration>
    int warm_up(Iteration &&iteration) {
        SBTV_TRY(refresh_spectra());
        SBTV_TRY(upload_lam_sigma());
        if (op->warmup > 0) {
            SBTV_TRY(do_prox(false));
            SBTV_TRY(operator_pass(true));                       // grad for the first step
            for (int ii = 2; ii <= op->warmup; ++ii) SBTV_TRY(iteration(ii));
        } else {
            SBTV_TRY(operator_pass(true));
        }
        SBTV_TRY(collect_scalars(0));
        SBTV_TRY(wait_scalars());
        for (int b = 0; b < batch; ++b) logpi0[b] = sapg_logpi(u, chain[b], scal_h, b);              // :131
        if (mom_sample_of(mom, 1)) SBTV_TRY(moments_seed(ctx, X, pm_mean, pm_m2, P, batch));          // iteration 1
        if (!dev_loop) SBTV_TRY(upload_lam_sigma());             // replayed warm-up iterations restaged the whole block
        return do_prox(false);                                   // proxGX = proxG(X, thetas(1))   (:134)
    }

    // the traces and chains (on the host, or on their way there), EB means (:258-284), last sample, posterior moments ->
    // the caller's arrays
    int finish() {
        const int samples = u.samples;
        if (x_last) {
            if (flags & SBTV_DEVICE_PTRS)
                SBTV_HIP(ctx, hipMemcpyAsync(x_last, X, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
            else
                SBTV_TRY(stage_out_copy(ctx, x_last, X, cnt, flags));
        }
        if (mom) SBTV_TRY(moments_finish(ctx, pm_mean, pm_m2, P, batch, mom_count(*mom, samples), *mom));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        sapg_copy_out(u, op, tr.data(), chain.data(), logpi0.data(), SapgOut{thetas, ps, sigmas, logpi, logpi_wu, gx, grads, eb});
        return canary_epilogue(ctx, 0);
    }

    // ================= device-resident loop: warm-up (:66-93), SAPG iterations (:98-248) =================
    // the body, then the update kernel(s) with the in-stream collective between them, then the redo launch of the prox
    int device_iteration(bool main, bool respec, bool in_graph) {
        SBTV_TRY(iteration_body(main, respec, in_graph));
        if (!main) {
            SBTV_TRY(update(SAPG_PH_WARMUP));
        } else if (!in_stream()) {
            SBTV_TRY(update(SAPG_PH_GRADS | SAPG_PH_UPDATE));
        } else {
            SBTV_TRY(update(SAPG_PH_GRADS));
            if (reinterpret_cast<sbtv_allreduce_dev_fn>(reduce_fn)(reduce_user, u.red, 6, (void *)ctx->stream) != 0) {
                reduce_broken = true;              // the collective itself failed: nothing left to keep in step with
                return fail(ctx, SBTV_ERR_BADARG, "SAPG_algorithm: reduce_fn failed");
            }
            collective_done = true;
            SBTV_TRY(update(SAPG_PH_UPDATE));
        }
        // the prox's stop rule has been applied by the update kernel: re-run the steps up to an early stop
        if (defer_rule) SBTV_TRY(prox_iterate(ctx, pp, X, op->chambolleit, prox, true, 4));
        return 0;
    }
    // iteration ii, replayed or eagerly: the captured body takes everything from device memory, so launches need no staging
    int device_step(bool main, int ii) {
        bool replayed = false;
        if (ii >= 3)
            SBTV_TRY(replay(&graphs.g[main], &replayed, [&] { return device_iteration(main, main && params_move, true); },
                            [&] {
                                ++noise_step;            // the device counter advances by itself; keep the host's in step
                                return 0;
                            }));
        return replayed ? 0 : device_iteration(main, main && params_move && ii > 2, false);
    }
    int peer_failed() {          // after a synchronisation: has any rank reported a failure?
        if (!in_stream()) return 0;
        double latch = 0.0;
        SBTV_HIP(ctx, hipMemcpy(&latch, u.red + 6, sizeof(double), hipMemcpyDeviceToHost));
        return latch != 0.0 ? fail(ctx, SBTV_ERR_PEER, "SAPG_algorithm: another rank reported an error through reduce_fn") : 0;
    }
    int device_loop() {
        const int samples = u.samples;
        double *delta_d = nullptr, *tr_d = nullptr;
        SBTV_TRY(ws_get_t(ctx, "sapg.delta", (size_t)samples + 1, &delta_d));
        SBTV_TRY(ws_get_t(ctx, "sapg.red", 8, &u.red));
        SBTV_TRY(ws_get_t(ctx, "sapg.G", 4 * (size_t)batch, &u.G));
        SBTV_TRY(ws_get_t(ctx, "sapg.traces", tr.size(), &tr_d));
        SBTV_TRY(ws_get_t(ctx, "sapg.chain", (size_t)batch, &u.chain));
        SBTV_TRY(ws_get_t(ctx, "sapg.it", 2, &u.it));
        u.scal = scal_d; u.par = par; u.delta = delta_d; u.tr = sapg_traces(tr_d, u);
        {
            const int nlp = prox_launches(pp, op->chambolleit);
            u.pctrl = defer_rule ? pp.ctrl : nullptr;
            u.prox_k = op->chambolleit; u.prox_base = op->chambolleit / nlp; u.prox_extra = op->chambolleit % nlp;
        }
        // constants and initial chain state
        {
            std::vector<double> dl((size_t)samples + 1, 0.0);
            for (int ii = 2; ii <= samples; ++ii) dl[ii] = sapg_delta(op, u.dimX, ii);
            const int it0[2] = {2, 2};
            SBTV_HIP(ctx, hipMemcpyAsync(delta_d, dl.data(), sizeof(double) * dl.size(), hipMemcpyHostToDevice, ctx->stream));
            SBTV_HIP(ctx, hipMemcpyAsync(u.chain, chain.data(), sizeof(SapgChain) * batch, hipMemcpyHostToDevice, ctx->stream));
            SBTV_HIP(ctx, hipMemcpyAsync(u.it, it0, sizeof(it0), hipMemcpyHostToDevice, ctx->stream));
            SBTV_HIP(ctx, hipMemsetAsync(tr_d, 0, sizeof(double) * tr.size(), ctx->stream));
            SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the staging vector goes out of scope
        }
        SBTV_TRY(warm_up([&](int ii) -> int {
            SBTV_TRY(device_step(false, ii));
            if ((ii & 1023) == 0) SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            return 0;
        }));
        // In-stream collective (SBTV_REDUCE_DEVICE): the host runs up to 1024 iterations ahead of the device, so a rank
        // that fails locally cannot simply return - its peers have already enqueued, or will enqueue, one all-reduce per
        // remaining iteration and would wait for it inside the collective.  Such a rank keeps calling reduce_fn once per
        // remaining iteration with {0, 0, 0, 0, 0 chains, 1 failed} and only then returns its error; the peers latch the
        // flag on the device (red[6]) and return SBTV_ERR_PEER at their next synchronisation.  Only when reduce_fn
        // itself fails does a rank return at once.
        int local_rc = 0;
        std::string local_err;
        if (in_stream()) SBTV_HIP(ctx, hipMemsetAsync(u.red, 0, sizeof(double) * 8, ctx->stream));
        // test hook: SBTV_TEST_FAIL_SAPG="ii:chain_offset" makes the call whose first chain is `chain_offset` fail locally
        // at SAPG iteration ii (how tests exercise the failure protocol of the in-stream collective)
        int inject_ii = -1;
        if (const char *e = getenv("SBTV_TEST_FAIL_SAPG")) {
            int a = 0, b = 0;
            if (sscanf(e, "%d:%d", &a, &b) == 2 && b == op->chain_offset) inject_ii = a;
        }
        for (int ii = 2; ii <= samples; ++ii) {
            collective_done = false;
            main_ii = ii;
            if (local_rc == 0) {
                int rc = (ii == inject_ii) ? fail(ctx, SBTV_ERR_NOMEM, "SAPG_algorithm: injected failure (SBTV_TEST_FAIL_SAPG)") : 0;
                if (rc == 0) rc = device_step(true, ii);
                if (rc != 0) {
                    if (!in_stream() || reduce_broken) return rc;
                    local_rc = rc;
                    local_err = ctx->err;
                }
            }
            if (local_rc != 0 && !collective_done) {
                static const double failed_vec[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
                if (hipMemcpyAsync(u.red, failed_vec, sizeof(failed_vec), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                    reinterpret_cast<sbtv_allreduce_dev_fn>(reduce_fn)(reduce_user, u.red, 6, (void *)ctx->stream) != 0)
                    break;
            }
            if ((ii & 1023) == 0) {
                SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
                if (local_rc == 0) SBTV_TRY(peer_failed());
            }
        }
        if (local_rc != 0) {
            (void)hipStreamSynchronize(ctx->stream);
            return fail(ctx, local_rc, local_err);
        }
        if (in_stream()) {
            SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            SBTV_TRY(peer_failed());
        }
        SBTV_HIP(ctx, hipMemcpyAsync(tr.data(), tr_d, sizeof(double) * tr.size(), hipMemcpyDeviceToHost, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(chain.data(), u.chain, sizeof(SapgChain) * batch, hipMemcpyDeviceToHost, ctx->stream));
        return finish();
    }

    // ================= host-side loop: the host waits for the scalars of every iteration and steps the chains =================
    // Device work of one iteration up to the scalars on the host.  A replayed iteration reads every per-iteration value
    // (taps, lambda*theta, sigma^2, noise step) from the device parameter block, which the graph's first node refreshes
    // from the pinned staging block; staging needs no synchronisation, the wait that ended the previous iteration is one.
    int host_iteration(bool main, int ii) {
        bool replayed = false;
        if (ii >= 3)
            SBTV_TRY(replay(&graphs.g[main], &replayed,
                            [&]() -> int {
                                SBTV_HIP(ctx, hipMemcpyAsync(par, par_h, sizeof(double) * npar_all, hipMemcpyHostToDevice, ctx->stream));
                                return iteration_body(main, main && params_move, true);
                            },
                            [&]() -> int {
                                if (main && params_move) SBTV_TRY(stage_taps());
                                stage_lam_sigma();
                                par_h[npar_all - 1] = (double)noise_step;
                                ++noise_step;
                                return 0;
                            }));
        if (replayed) return wait_stream(ctx);
        if (main) SBTV_TRY(upload_lam_sigma());                                                    // theta(ii-1), sigma(ii-1)
        SBTV_TRY(iteration_body(main, main && params_move && ii > 2, false));
        return wait_scalars();
    }
    int host_loop() {
        const int samples = u.samples;
        const SapgTraces h = sapg_traces(tr.data(), u);
        SBTV_TRY(warm_up([&](int ii) -> int {
            SBTV_TRY(host_iteration(false, ii));
            for (int b = 0; b < batch; ++b) h.wu[(size_t)b * u.warmup + (ii - 1)] = sapg_logpi(u, chain[b], scal_h, b);   // :85
            return 0;
        }));
        std::vector<double> G(4 * (size_t)batch, 0.0);
        for (int ii = 2; ii <= samples; ++ii) {
            main_ii = ii;
            // In the shared-gradient mode a failure of the device work must not return at once: the peer ranks are about to
            // enter this iteration's all-reduce and would wait for ever, so the status travels with the gradients (sixth
            // reduced element) and every rank leaves together.
            const int rc_dev = host_iteration(true, ii);
            if (rc_dev != 0 && !(u.shared && reduce_fn)) return rc_dev;
            for (int b = 0; b < batch && rc_dev == 0; ++b) sapg_gradients(u, h, chain[b], scal_h, b, ii, &G[4 * (size_t)b]);
            if (u.shared) {
                // all chains sample the same posterior: average their gradients (the reference's
                // `for jj=1:1 ... G = mean(g_*)`, SAPG_algorithm_moffat.m:158-173), across ranks too
                // [sum G_theta, sum G_p0, sum G_p1, sum G_sigma, chains, ranks that failed in this iteration]
                double buf[6] = {0, 0, 0, 0, (double)batch, rc_dev != 0 ? 1.0 : 0.0};
                for (int b = 0; b < batch && rc_dev == 0; ++b)
                    for (int q = 0; q < 4; ++q) buf[q] += G[4 * (size_t)b + q];
                if (reduce_fn) {
                    int rc = reduce_fn(reduce_user, buf, 6);
                    if (rc_dev != 0) return rc_dev;            // the local error, after the peers have been told
                    if (rc != 0) return fail(ctx, SBTV_ERR_BADARG, "SAPG_algorithm: reduce_fn failed");
                    if (buf[5] != 0.0)
                        return fail(ctx, SBTV_ERR_PEER, "SAPG_algorithm: a peer rank of the shared-gradient chains failed in this iteration");
                }
                for (int b = 0; b < batch; ++b)
                    for (int q = 0; q < 4; ++q) G[4 * (size_t)b + q] = buf[q] / buf[4];
            }
            const double delta = sapg_delta(op, u.dimX, ii);
            for (int b = 0; b < batch; ++b) sapg_step(u, h, chain[b], b, ii, delta, &G[4 * (size_t)b]);
        }
        return finish();
    }
};

int sapg_impl(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const sbtv_sapg_opts *op, const double *x0,
              const double *noise, double *thetas, double *ps, double *sigmas, double *logpi, double *logpi_wu, double *gx,
              double *grads, double *eb, double *x_last, sbtv_allreduce_fn reduce_fn, void *reduce_user, int flags,
              const MomReq *mom) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(sapg_refuse(ctx, "SAPG_algorithm", y, M, N, batch, op));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    const int shared = op->share_gradients ? 1 : 0;
    // independent chains (SAPG_algorithm_moffat.m:143-173: every chain has its own state) -> two lanes of this context;
    // shared-gradient chains only in lanes_mode 2 (their per-iteration exchange couples the two streams).  Not when the
    // caller reduces across processes itself, forces the host loop, or injects device-resident noise (re-packed per lane).
    if (!reduce_fn && !(flags & (SBTV_SAPG_HOST_LOOP | SBTV_REDUCE_DEVICE)) && !(noise && (flags & SBTV_DEVICE_PTRS))) {
        if (sbtv_group *lg = lanes_group(ctx, batch, shared != 0)) {
            LaneCall lc(ctx, lg);
            if (!mom || !mom->pooled)
                return lc.done(sapg_sharded(lg, y, M, N, batch, op, x0, noise, thetas, ps, sigmas, logpi, logpi_wu, gx, grads,
                                            eb, x_last, flags, mom), batch);
            // pooled moments: every lane hands its chains' mean / M2 to this context, which pools them in chain order
            // afterwards (the same arithmetic as on one stream)
            const size_t cntl = (size_t)M * N * batch;
            double *lm = nullptr, *l2 = nullptr;
            SBTV_TRY(ws_get_t(ctx, "sapg.pm_lanes_mean", cntl, &lm));
            SBTV_TRY(ws_get_t(ctx, "sapg.pm_lanes_m2", cntl, &l2));
            MomReq lr = *mom;
            lr.mean = lm;
            lr.var = l2;
            lr.count = nullptr;
            lr.dev = true;
            lr.raw = true;
            SBTV_TRY(lc.done(sapg_sharded(lg, y, M, N, batch, op, x0, noise, thetas, ps, sigmas, logpi, logpi_wu, gx, grads, eb,
                                          x_last, flags, &lr), batch));
            SBTV_TRY(moments_finish(ctx, lm, l2, (size_t)M * N, batch, mom_count(*mom, op->samples), *mom));
            SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            return canary_epilogue(ctx, 0);
        }
    }
    SapgRun r{ctx, y, M, N, batch, op, x0, noise, thetas, ps, sigmas, logpi, logpi_wu, gx, grads, eb, x_last, reduce_fn,
              reduce_user, flags, mom};
    SBTV_TRY(r.setup());
    return r.dev_loop ? r.device_loop() : r.host_loop();
}

}  // namespace sbtv

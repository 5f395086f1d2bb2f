// FISTA (SALSA/my_fista.m, my_deblur_fista.m) and the power iteration (utils/max_eigenval_*.m) as device-resident
// loops over the TV-prox and spectral-operator kernels.
#include <cmath>
#include <cstring>

#include "sbtv_internal.h"

namespace sbtv {

__global__ __launch_bounds__(256) void scale_kernel(double *__restrict__ x, double a, size_t n2) {
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n2; q += (size_t)gridDim.x * 256) {
        double2 v = reinterpret_cast<double2 *>(x)[q];
        v.x *= a;
        v.y *= a;
        reinterpret_cast<double2 *>(x)[q] = v;
    }
}

static int launch_scale(sbtv_ctx *ctx, double *x, double a, size_t n) {
    hipLaunchKernelGGL(scale_kernel, dim3(ew_blocks(n)), dim3(256), 0, ctx->stream, x, a, n / 2);
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

// FISTA scalars of one iteration in one launch: block (q, b): q < 3 rows-kernel accumulators [batch][3][nrb] ->
// out[b*3+q]; q = 3..5 momentum-kernel sums [batch][3][npb] (may be null) -> out[3*batch + b*3 + (q-3)];
// q = 6 periodic-TV partials [batch][ntv] -> out[6*batch + b].  `out` is the device view of pinned host memory.
__global__ __launch_bounds__(256) void fista_collect_kernel(const double *__restrict__ acc, int nrb,
                                                            const double *__restrict__ mom, int npb,
                                                            const double *__restrict__ tvp, int ntv,
                                                            double *__restrict__ out, int batch,
                                                            const double *__restrict__ ppart, int pnblk,
                                                            unsigned long long tags_addr, double seq) {
    // tags [batch][8 + FSTRIDE] (pinned host memory, passed as an integer like the SALSA collector's): tag q (or 8 + s
    // for the step sums) = the iteration whose value `out` now holds; the host polls them instead of synchronising
    double *__restrict__ tags = reinterpret_cast<double *>(tags_addr);
    __shared__ double red[4];
    const int q = blockIdx.x, b = blockIdx.y;
    const double *p = nullptr;
    int n = 0;
    size_t o, t = (size_t)b * (8 + FSTRIDE) + q;
    double s = 0.0;
    if (q >= 7) {
        // optimistic prox launches (prox_iterate, spec): block 7 + s totals the error partials of Chambolle step s into
        // out[8*batch + b*FSTRIDE + s]; the host applies the stop rule of chambolle_prox_TV_stop.m:131 over the steps
        const int st = q - 7;
        s = step_sum_part(ppart + ((size_t)b * FSTRIDE + st) * pnblk, pnblk);
        o = 8 * (size_t)batch + (size_t)b * FSTRIDE + st;
        t = (size_t)b * (8 + FSTRIDE) + 8 + st;
    } else if (q < 3) {
        p = acc + ((size_t)b * 3 + q) * nrb;
        n = nrb;
        o = (size_t)b * 3 + q;
    } else if (q < 6) {
        p = mom ? mom + ((size_t)b * 3 + (q - 3)) * npb : nullptr;
        n = npb;
        o = 3 * (size_t)batch + (size_t)b * 3 + (q - 3);
    } else {
        p = tvp + (size_t)b * ntv;
        n = ntv;
        o = 6 * (size_t)batch + b;
    }
    if (p)
        for (int i = threadIdx.x; i < n; i += 256) s += p[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[o] = (red[0] + red[1]) + (red[2] + red[3]);
        if (tags) {
            __threadfence_system();
            __hip_atomic_store(&tags[t], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace sbtv

using namespace sbtv;

extern "C" {

// ---------------------------------------------------------------------------
// a-9: power iteration on A'A
// ---------------------------------------------------------------------------
int sbtv_max_eigenval(sbtv_ctx *ctx, const double *taps, int taille, const double *x0, int M, int N, double tol,
                      int max_iter, double *val_out, int *iters, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!taps || !x0 || !val_out) return fail(ctx, SBTV_ERR_BADARG, "max_eigenval: bad arguments");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    SBTV_TRY(check_even_pixels(ctx, M, N));
    BlurOp op;
    SBTV_TRY(op_open(ctx, "ev", M, N, 1, nullptr, &op));
    const size_t P = op.P;
    const double *x0d = nullptr;
    SBTV_TRY(stage_in(ctx, "ev.x0", x0, P, flags, &x0d));
    double *x = nullptr, *taps_d = nullptr, *o4 = nullptr;
    SBTV_TRY(ws_get_t(ctx, "ev.x", P, &x));
    SBTV_TRY(ws_get_t(ctx, "ev.taps", (size_t)taille * taille, &taps_d));
    SBTV_TRY(ws_get_t(ctx, "ev.o4", 4, &o4));
    SBTV_HIP(ctx, hipMemcpyAsync(taps_d, taps, sizeof(double) * taille * taille, hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(x, x0d, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(psf_spectrum(ctx, op.fp, taps_d, taille, op.Hs));
    double h4[4];
    auto norm_x = [&](double *nrm) -> int {
        SBTV_TRY(pair_sums(ctx, x, nullptr, P, 1, o4));
        SBTV_HIP(ctx, hipMemcpyAsync(h4, o4, sizeof(h4), hipMemcpyDeviceToHost, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *nrm = sqrt(h4[1]);
        return 0;
    };
    double nrm = 0.0;
    SBTV_TRY(norm_x(&nrm));
    SBTV_TRY(launch_scale(ctx, x, 1.0 / nrm, P));              // x = x / norm(x(:))          (:5)
    double init_val = 1.0, val = 1.0;
    int k = 0;
    for (k = 1; k <= max_iter; ++k) {
        SBTV_TRY(op_apply(ctx, op, OP_ATA, x, x));              // y = A(x); x = At(y)        (:9-10)
        SBTV_TRY(norm_x(&val));                                 // val = norm(x(:))            (:11)
        const double rel_var = fabs(val - init_val) / init_val;
        if (rel_var < tol) break;                               //                            (:16-18)
        init_val = val;
        SBTV_TRY(launch_scale(ctx, x, 1.0 / val, P));          // x = x / val                (:20)
    }
    *val_out = val;
    if (iters) *iters = (k > max_iter) ? max_iter : k;
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// a-8: FISTA with Psi = cold-start Chambolle, Phi = periodic TVnorm
// ---------------------------------------------------------------------------
// one solve on the staged inputs (device pointers bd, td); spec_wanted: optimistic prox launches
static int fista_solve(sbtv_ctx *ctx, const double *bd, int M, int N, int batch, const double *taps, int taille,
                       const double *tau, double L, int prox_iters, int stopcriterion, double tolerance, int maxiters,
                       int zero_start, const double *td, double *x_out, double *objective, double *mses, int *n_iter,
                       int flags, bool spec_wanted) {
    BlurOp op;                                          // its observation spectrum: "fista.B"
    SBTV_TRY(op_open(ctx, "fista", M, N, batch, "B", &op));
    const FftPlan &fp = op.fp;
    double2 *const S = op.S;
    ProxPlan pp;
    SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
    const size_t P = op.P, cnt = P * batch;
    // x is double-buffered by iteration parity: the host evaluates the stopping rule one iteration late while the next
    // iteration already runs, and the iterate of a stopping iteration must still be intact then
    double *xb[2] = {nullptr, nullptr}, *y = nullptr, *grad = nullptr, *xfinal = nullptr;
    SBTV_TRY(ws_get_t(ctx, "fista.x", cnt, &xb[1]));
    SBTV_TRY(ws_get_t(ctx, "fista.x2", cnt, &xb[0]));
    double *x = xb[1];                                  // iterate 1 (the start)
    SBTV_TRY(ws_get_t(ctx, "fista.y", cnt, &y));
    SBTV_TRY(ws_get_t(ctx, "fista.grad", cnt, &grad));
    SBTV_TRY(stage_out_buf(ctx, "fista.xfinal", x_out, cnt, flags, &xfinal));
    const size_t npar = (size_t)batch * taille * taille + 2 * (size_t)batch;
    double *par = nullptr;
    SBTV_TRY(ws_get_t(ctx, "fista.par", npar, &par));
    double *taps_d = par, *lam_d = par + (size_t)batch * taille * taille;
    std::vector<double> hpar(npar);
    for (size_t q = 0; q < (size_t)batch * taille * taille; ++q) hpar[q] = taps[q];
    for (int b = 0; b < batch; ++b) {
        hpar[(size_t)batch * taille * taille + b] = tau[b] / L;     // Psi(y, tau/L)   (my_fista.m:26)
        hpar[(size_t)batch * taille * taille + batch + b] = 0.0;
    }
    SBTV_HIP(ctx, hipMemcpyAsync(par, hpar.data(), sizeof(double) * npar, hipMemcpyHostToDevice, ctx->stream));
    int *frozen_d = nullptr;
    SBTV_TRY(ws_get_t(ctx, "fista.frozen", (size_t)batch, &frozen_d));
    SBTV_HIP(ctx, hipMemsetAsync(frozen_d, 0, sizeof(int) * batch, ctx->stream));
    const int nrb = fft_rows_blocks(fp), npb = ew_blocks(P);
    double *acc = nullptr, *momp = nullptr, *o4 = nullptr;
    SBTV_TRY(ws_get_t(ctx, "fista.acc", (size_t)batch * 3 * nrb, &acc));
    SBTV_TRY(ws_get_t(ctx, "fista.momp", (size_t)batch * 3 * npb, &momp));
    SBTV_TRY(ws_get_t(ctx, "fista.o4", (size_t)batch * 4, &o4));
    // pinned: two slots (iteration parity) of [acc3 | mom3 | tv | pad] per image + the step sums of an optimistic prox,
    // then their completion tags, then the frozen flags for upload; host / device view
    constexpr int FT = 8 + FSTRIDE;
    const size_t slot_n = (size_t)FT * batch;
    PinnedLayout lay;
    const auto f_scal = lay.add<double>(2 * slot_n), f_tags = lay.add<double>(2 * slot_n);
    const auto f_frozen = lay.add<int>((size_t)batch);
    void *ph = nullptr, *pd = nullptr;
    SBTV_TRY(pinned_get(ctx, lay.bytes(), &ph, &pd));
    double *scal_base_h = f_scal.at(ph), *scal_base_hd = f_scal.at(pd);
    double *tags_base_h = f_tags.at(ph), *tags_base_hd = f_tags.at(pd);
    int *frozen_h = f_frozen.at(ph);
    for (size_t i = 0; i < f_tags.count; ++i) tags_base_h[i] = 0.0;               // tags: no iteration yet
    for (int b = 0; b < batch; ++b) frozen_h[b] = 0;
    SBTV_TRY(psf_spectrum(ctx, fp, taps_d, taille, op.Hs));
    SBTV_TRY(op_spectrum(ctx, fp, bd, nullptr, S, op.Ys));
    // x = AT(b) (my_fista.m:7) or zeros (my_deblur_fista.m:21)
    SBTV_TRY(op_init_x(ctx, op, zero_start ? 0 : 2, bd, nullptr, x));
    SBTV_HIP(ctx, hipMemcpyAsync(y, x, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));

    // objective(k) = 0.5*||A x - b||^2 + tau*Phi(x) ; mses(k)   (:14-15, :31-33)
    // residual energy (Parseval) and TV partials of x, then ONE collector launch that reduces them (and the
    // momentum-kernel sums when given) straight into pinned host memory
    // Optimistic prox launches (no stop-rule kernels, no redo pass: 6 launches less per iteration); the host applies the
    // rule over the prox_iters step sums when it reads the iteration's scalars and, should it have stopped early, repeats
    // the whole solve with exact launches, so the result is always that of the exact rule.
    // (not when a device-resident x_out overlaps an input: frozen images are copied into x_out while the loop runs, and a
    // repeated solve would then start from damaged inputs - such a call takes the exact launches from the start)
    const bool out_aliases_input = (flags & SBTV_DEVICE_PTRS) && (overlaps(bd, x_out, cnt) || overlaps(td, x_out, cnt));
    const bool prox_spec = spec_wanted && !out_aliases_input && prox_spec_ok(pp, y, x, prox_iters);
    bool prox_was_spec = false;
    // objective / sums of iterate `xk` of iteration k -> pinned slot k & 1, tagged with k
    auto objective_of_x = [&](const double *xk, int k, const int *frozen, const double *mom_partials) -> int {
        // TVnorm(x) rides on the forward column pass over the same image (no TV launch of its own)
        double *tvp = nullptr;
        int ntv = 0;
        if (fft_cols_tv_ok(fp)) {
            ntv = fft_cols_blocks(fp);
            SBTV_TRY(ws_get_t(ctx, "fista.tvc", (size_t)batch * ntv, &tvp));
        }
        SBTV_TRY(op_resid(ctx, op, xk, acc, frozen, tvp));
        if (!tvp) SBTV_TRY(tvnorm_partials(ctx, xk, M, N, batch, &tvp, &ntv));
        const int slot = k & 1;
        hipLaunchKernelGGL(fista_collect_kernel, dim3(prox_was_spec ? 7 + prox_iters : 7, batch), dim3(256), 0, ctx->stream,
                           (const double *)acc, nrb, mom_partials, npb, (const double *)tvp, ntv, scal_base_hd + slot * slot_n,
                           batch, (const double *)pp.partials, pp.fnblk,
                           (unsigned long long)(uintptr_t)(tags_base_hd + slot * slot_n), (double)k);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    };
    std::vector<double> obj_prev(batch, 0.0);
    std::vector<int> frozen(batch, 0), h_niter(batch, 1);
    SBTV_TRY(objective_of_x(x, 1, nullptr, nullptr));
    SBTV_TRY(pair_sums(ctx, x, td, P, batch, o4));
    {
        std::vector<double> h4((size_t)batch * 4);
        SBTV_HIP(ctx, hipMemcpyAsync(h4.data(), o4, sizeof(double) * 4 * batch, hipMemcpyDeviceToHost, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const double *sc = scal_base_h + slot_n;       // slot of iteration 1
        for (int b = 0; b < batch; ++b) {
            const double f0 = 0.5 * (sc[(size_t)b * 3] * op.parseval) + tau[b] * sc[6 * (size_t)batch + b];
            obj_prev[b] = f0;
            if (objective) objective[(size_t)b * maxiters] = f0;
            if (mses) mses[(size_t)b * maxiters] = h4[(size_t)b * 4] / (double)P;
        }
    }
    // The loop keeps one iteration in flight beyond the one the host is looking at (SBTV_FISTA_LAG=0: none): iteration
    // k + 1 is enqueued before the scalars of iteration k are read, so the GPU never waits for the host.  If iteration k
    // turns out to be an image's last, its iterate is still intact in its half of the double buffer (iteration k + 1
    // wrote the other half), and whatever k + 1 did to that image is ignored.
    static const int lag = [] {
        const char *e = getenv("SBTV_FISTA_LAG");
        return (e && e[0] == '0') ? 0 : 1;
    }();
    double t_enq = 1.0;
    int active = batch;
    bool slot_spec[2] = {false, false};
    // fused gradient step (SBTV_FISTA_FUSED_STEP=0: the two-pass form, for A/B runs)
    static const bool fused_wanted = [] {
        const char *e = getenv("SBTV_FISTA_FUSED_STEP");
        return !(e && e[0] == '0');
    }();
    const bool fused_step = fused_wanted && prox_spec && fft_cols_inv_step_ok(fp);
    if (fused_step) SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, prox_iters, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, frozen_d));
    auto enqueue = [&](int k) -> int {
        const double t_old = t_enq;
        double *xk = xb[k & 1];
        // y = y - (1/L) * AT(A(y) - b)                                   (:25)
        {
            RowsArgs a{};
            a.dir_fwd = 1;
            a.dir_inv = 1;
            a.op = OP_GRADF;
            a.H = op.Hs;
            a.Y = op.Ys;
            a.acc = acc;
            a.frozen = frozen_d;
            SBTV_TRY(fft_cols_fwd_f(ctx, fp, y, nullptr, S, frozen_d));
            SBTV_TRY(fft_rows(ctx, fp, S, S, a));
            if (fused_step) {
                // the gradient never reaches memory: the inverse column pass applies the step to y from its registers
                // (optimistic prox launches do not consult the control blocks: armed once before the loop)
                SBTV_TRY(fft_cols_inv_step(ctx, fp, S, y, op.inv_scale, 1.0 / L, frozen_d));
            } else {
                SBTV_TRY(fft_cols_inv_f(ctx, fp, S, grad, op.inv_scale, frozen_d));
                // the gradient-step kernel also re-arms the control blocks of the cold-start prox that follows
                const ProxArm arm{pp.ctrl, lam_d, prox_iters, CHAMBOLLE_TOL, CHAMBOLLE_TAU, frozen_d};
                if (batch <= 256) {
                    SBTV_TRY(axpy(ctx, y, grad, 1.0 / L, cnt, &arm, batch));
                } else {
                    SBTV_TRY(axpy(ctx, y, grad, 1.0 / L, cnt));
                    SBTV_TRY(prox_reset(ctx, pp, lam_d, 1.0, prox_iters, CHAMBOLLE_TOL, CHAMBOLLE_TAU, false, frozen_d));
                }
            }
        }
        // x = Psi(y, tau/L): cold-start Chambolle                        (:26 ; run_moffat_demo.m:181-182)
        prox_was_spec = prox_spec;
        slot_spec[k & 1] = prox_spec;
        SBTV_TRY(prox_iterate(ctx, pp, y, prox_iters, xk, true, prox_spec));
        t_enq = 0.5 * (1 + sqrt(1 + 4 * t_old * t_old));                 // :28
        SBTV_TRY(fista_momentum(ctx, xk, xb[(k - 1) & 1], y, td, (t_old - 1) / t_enq, momp, P, batch, frozen_d));   // :29-30
        SBTV_TRY(objective_of_x(xk, k, frozen_d, momp));
        return 0;
    };
    auto process = [&](int k) -> int {
        // until the collector of iteration k has delivered every scalar (and the step sums) of every image
        SBTV_TRY(wait_tags(ctx, tags_base_h + (size_t)(k & 1) * slot_n, batch, FT, 7, slot_spec[k & 1] ? prox_iters : 0,
                           (double)k));
        const double *sc = scal_base_h + (size_t)(k & 1) * slot_n;
        // the stop rule of the optimistic prox with the tolerance armed above: fired before the last step -> start over
        if (slot_spec[k & 1])
            SBTV_TRY(spec_stop_rule(ctx, pp, sc + 8 * (size_t)batch, prox_iters, CHAMBOLLE_TOL, frozen.data()));
        bool changed = false;
        for (int b = 0; b < batch; ++b) {
            if (frozen[b]) continue;
            const double f = 0.5 * (sc[(size_t)b * 3] * op.parseval) + tau[b] * sc[6 * (size_t)batch + b];
            const double *mom = sc + 3 * (size_t)batch + (size_t)b * 3;
            if (objective) objective[(size_t)b * maxiters + (k - 1)] = f;
            if (mses) mses[(size_t)b * maxiters + (k - 1)] = mom[0] / (double)P;
            h_niter[b] = k;
            double crit;
            if (stopcriterion == 1)
                crit = fabs(f - obj_prev[b]) / f;                        // :38 (divides by objective(k))
            else if (stopcriterion == 2)
                crit = sqrt(mom[1]) / sqrt(mom[2]);                      // :40
            else
                crit = f;                                                // :42
            obj_prev[b] = f;
            if (crit < tolerance) {                                      // :51
                frozen[b] = 1;
                frozen_h[b] = 1;
                --active;
                changed = true;
                SBTV_HIP(ctx, hipMemcpyAsync(xfinal + (size_t)b * P, xb[k & 1] + (size_t)b * P, sizeof(double) * P,
                                             hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        // with the fused step nothing re-arms the control blocks per iteration: park the frozen images' prox
        if (changed && active > 0) SBTV_TRY(upload_frozen(ctx, frozen_h, frozen_d, batch, fused_step ? pp.ctrl : nullptr));
        return 0;
    };
    int done = 1;
    SBTV_TRY(pipelined_loop(ctx, &done, maxiters, lag, true, enqueue, process, [&] { return active > 0; }));
    for (int b = 0; b < batch; ++b)
        if (!frozen[b])
            SBTV_HIP(ctx, hipMemcpyAsync(xfinal + (size_t)b * P, xb[h_niter[b] & 1] + (size_t)b * P, sizeof(double) * P,
                                         hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(stage_out_copy(ctx, x_out, xfinal, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_iter)
        for (int b = 0; b < batch; ++b) n_iter[b] = h_niter[b];
    return 0;
}

int sbtv_fista_tv(sbtv_ctx *ctx, const double *bimg, int M, int N, int batch, const double *taps, int taille,
                  const double *tau, double L, int prox_iters, int stopcriterion, double tolerance, int maxiters,
                  int zero_start, const double *true_x, double *x_out, double *objective, double *mses, int *n_iter,
                  int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!bimg || !taps || !tau || !true_x || batch < 1 || maxiters < 1 || !(L > 0.0))
        return fail(ctx, SBTV_ERR_BADARG, "fista_tv: bad arguments (b, taps, tau, true are required)");
    if (stopcriterion < 1 || stopcriterion > 3) return fail(ctx, SBTV_ERR_STOPCRITERION, "Invalid stopping criterion!");
    if (prox_iters <= 0) return fail(ctx, SBTV_ERR_MAXITER, "fista_tv: prox_iters must be positive");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    SBTV_TRY(check_even_pixels(ctx, M, N));
    if (sbtv_group *lg = lanes_group(ctx, batch, false)) {       // independent images: two lanes of this context (group.hip)
        LaneCall lc(ctx, lg);
        return lc.done(fista_sharded(lg, bimg, M, N, batch, taps, taille, tau, L, prox_iters, stopcriterion, tolerance, maxiters,
                                     zero_start, true_x, x_out, objective, mses, n_iter, flags), batch);
    }
    const size_t cnt = (size_t)M * N * batch;
    const double *bd = nullptr, *td = nullptr;
    SBTV_TRY(stage_in(ctx, "fista.b", bimg, cnt, flags, &bd));
    SBTV_TRY(stage_in(ctx, "fista.true", true_x, cnt, flags, &td));
    // optimistic prox launches first, unless SBTV_FISTA_EXACT_PROX asks for exact ones; repeated exactly if the rule fired
    return canary_epilogue(ctx, solve_with_exact_repeat(ctx, !(flags & SBTV_FISTA_EXACT_PROX), [&](bool spec) {
        return fista_solve(ctx, bd, M, N, batch, taps, taille, tau, L, prox_iters, stopcriterion, tolerance, maxiters,
                           zero_start, td, x_out, objective, mses, n_iter, flags, spec);
    }));
}

// Device-resident SALSA_v2 (ADMM, SALSA/SALSA_v2.m:389-494) over the TV prox and the spectral
// blur operator.  The host only sees eight scalars per image and outer iteration (objective
// terms, mse, distance) and applies the stopping rule; images never leave HBM.
//
// One SALSA outer iteration (fused form):
//   u      = prox_{(tau/mu) TV}(x - bu)   warm-started duals       (:429)
//   S      = rfft2(u + bu)                                        (:434, FFT of mu*(u+bu) up to the factor)
//   Xh     = (conj(H) Yh + mu S) / (|H|^2 + mu)                   (:434-436; ATy enters as conj(H) Yh)
//   resid2 = sum |Yh - H Xh|^2 / (M N)          (Parseval for  :442-444, no second FFT pair)
//   x      = irfft2(Xh)
//   bu    += u - x ; g = x - bu ; sums for mse / distance / TVnorm(u)  (:440,444,446-451)
//
// Speculative pipelining: the host enqueues outer iteration k+1 before it has seen the scalars of
// iteration k, so the GPU never waits for the stop-rule round trip.  x is double-buffered, hence
// when iteration k turns out to be the last one its x is still intact (one wasted iteration).
#include <algorithm>
#include <chrono>
#include <cmath>

#include <time.h>

#include "sbtv_internal.h"

namespace sbtv {

// start of a call: per-image parameters from the pinned staging block into device memory, frozen flags cleared
__global__ void salsa_setup_kernel(const double *__restrict__ src, double *__restrict__ par, int npar, int *__restrict__ frozen,
                                   int batch) {
    for (int i = threadIdx.x; i < npar; i += blockDim.x) par[i] = src[i];
    for (int b = threadIdx.x; b < batch; b += blockDim.x) frozen[b] = 0;
}

// x = g + bu = (x - bu) + bu of an image's last iteration (NOX mode of sbtv_SALSA_v2: x is not stored in the loop)
__global__ __launch_bounds__(256) void salsa_recover_x_kernel(const double *__restrict__ g, const double *__restrict__ bu,
                                                               double *__restrict__ x, size_t P) {
#pragma clang fp contract(off)
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < P / 2; q += (size_t)gridDim.x * 256) {
        const double2 a = *reinterpret_cast<const double2 *>(g + 2 * q), b = *reinterpret_cast<const double2 *>(bu + 2 * q);
        *reinterpret_cast<double2 *>(x + 2 * q) = make_double2(a.x + b.x, a.y + b.y);
    }
}

// grid (7 [+ psteps], batch): see collect.inc (salsa_collect_block); the same blocks can ride on the first Chambolle
// launch of the next outer iteration instead (SideJob, tv_fused.inc)
__global__ __launch_bounds__(256) void salsa_collect_kernel(Collect c, ProxCtrl *__restrict__ ctrl,
                                                             unsigned long long out_addr,
                                                             const int *__restrict__ frozen, int rearm,
                                                             unsigned long long tags_addr, double seq) {
    __shared__ double red[4];
    salsa_collect_block(c, ctrl, out_addr, frozen, rearm, tags_addr, seq, blockIdx.x, blockIdx.y, red);
}

}  // namespace sbtv

using namespace sbtv;

extern "C" {

void sbtv_salsa_opts_default(sbtv_salsa_opts *o) {
    if (!o) return;
    o->stopcriterion = 1;      // SALSA_v2.m:171
    o->maxiter = 10000;        // :173
    o->TViters = 5;            // :181
    o->initialization = 0;     // :174
    o->compute_mse = 0;        // :172
    o->speculate = 1;
    o->tolA = 0.001;           // :178
    o->chambolle_tol = 1e-3;   // chambolle_prox_TV_stop.m:78
    o->chambolle_tau = 0.249;  // chambolle_prox_TV_stop.m:77
}

}  // extern "C"

namespace {

// One solve on the staged inputs (device pointers yd, td, xi): the arguments, the buffers, the phases before the loop, the
// two halves of an outer iteration (enqueue / process) and what follows the loop.  run() strings them together.
struct SalsaRun {
    // ---- the call (sbtv_SALSA_v2's arguments after staging); spec_wanted: optimistic prox launches
    sbtv_ctx *ctx; const double *yd; int M, N, batch; const double *taps; int taille; const double *tau, *mu;
    const sbtv_salsa_opts *opts; const double *td, *xi; double *x_out, *objective, *distance, *times, *mses;
    int *numA, *numAt, *n_outer; int flags; bool spec_wanted;

    // ---- plans, constants, buffers
    BlurOp op{};
    ProxPlan pp;
    size_t P = 0, cnt = 0, npar = 0;
    int maxiter = 0, lag = 0, nrb = 0, npb = 0, nl_prox = 0;
    bool want_mse = false, crit2 = false, zero_start = false, direct_last_ok = false, direct_last = false, nox = false,
         spec_ok = false, use_graph = false;
    double *xbuf[2] = {nullptr, nullptr}, *u = nullptr, *gb[2] = {nullptr, nullptr}, *bub[2] = {nullptr, nullptr};
    double *par = nullptr, *taps_d = nullptr, *mu_d = nullptr, *thr_d = nullptr;     // [taps | mu | thr] per image
    double *acc = nullptr, *postp = nullptr, *o4 = nullptr;
    int *frozen_d = nullptr;
    // the pinned block as the host (_h) and the device (_hd) see it; its fields in order: DESIGN.md section 3.12
    SalsaScal *scal_h = nullptr, *scal_hd = nullptr, *init_h = nullptr, *init_hd = nullptr;
    double *psum_h = nullptr, *psum_hd = nullptr, *tags_h = nullptr, *tags_hd = nullptr, *init_tags_h = nullptr,
           *init_tags_hd = nullptr;
    int *frozen_h = nullptr;
    hipEvent_t ev_done[2], ev_p0[2], ev_p1[2];

    // ---- state
    std::vector<int> h_numA, h_numAt, frozen, h_nouter;
    std::vector<double> obj_prev;
    bool init_read = false;
    int active = 0;
    double ms_prox = 0.0;
    long long prox_iters_run = 0, prox_iters_timed = 0;
    GraphExecs graphs;            // captured graphs of this call: released on EVERY return path
    std::chrono::steady_clock::time_point t0;
    bool prox_timed[2] = {false, false}, slot_tagged[2] = {false, false}, slot_spec[2] = {false, false};
    // The collector of an optimistic iteration does not get a launch of its own when another iteration follows: its
    // blocks ride on the first Chambolle launch of that next iteration (SideJob; a launch costs ~5 us however little
    // it does).  `pend` = the collector still to be placed.  Error partials alternate between two sets by iteration
    // parity, so the riding collector reads one set while its host launch already writes the other.
    struct PendingCollect {
        bool valid = false;
        int outer = 0;
        bool spec = false;
    } pend;

    // plans, buffers, the pinned block, parameter upload
    int open() {
        SBTV_TRY(op_open(ctx, "salsa", M, N, batch, "Y", &op));
        SBTV_TRY(prox_plan(ctx, M, N, batch, &pp));
        P = op.P;
        cnt = P * batch;
        maxiter = opts->maxiter;
        want_mse = (td != nullptr);
        crit2 = (opts->stopcriterion == 2);
        zero_start = (opts->initialization == 0);
        lag = (opts->speculate & 1) ? 1 : 0;
        SBTV_TRY(ws_get_t(ctx, "salsa.x0", cnt, &xbuf[0]));
        SBTV_TRY(ws_get_t(ctx, "salsa.x1", cnt, &xbuf[1]));
        // The last possible iteration (outer == maxiter) writes its x straight into a device-resident x_out: a solve that
        // runs to MAXITERA then ends without the copy out of the double buffer (images that stop earlier are copied as
        // before, after that write).  Not when x_out overlaps an input (an optimistic solve that has to be repeated reads
        // them again) and not with captured iterations (their arguments are frozen).
        direct_last_ok = x_out && (flags & SBTV_DEVICE_PTRS) && !graph_wanted(cnt) && !overlaps(yd, x_out, cnt) &&
                         !overlaps(td, x_out, cnt) && !overlaps(xi, x_out, cnt);
        SBTV_TRY(ws_get_t(ctx, "salsa.u", cnt, &u));
        SBTV_TRY(ws_get_t(ctx, "salsa.bu", cnt, &bub[0]));
        SBTV_TRY(ws_get_t(ctx, "salsa.g", cnt, &gb[0]));
        // NOX (sizes of the wave-granular column pass, stop criteria 1 and 3, eager launches): the inverse column pass does not
        // STORE x (one of the eight array passes of the bookkeeping kernel: -2.5 % of an outer iteration at 2048^2).  Nothing in
        // the loop reads x again; the final x of an image is recovered as g + bu = (x - bu) + bu of ITS last iteration, so g
        // and bu alternate between two buffers by iteration parity (the host learns one iteration late which one was the
        // last; x was double-buffered for the same reason).  The recovered x differs from the transform's output by the
        // rounding of that sum (<= 1 ulp of |x| + |bu|, ~3e-14 on 0..255 data).  SBTV_SALSA_NOX=0: store x.
        static const bool env_nox = [] {
            const char *e = getenv("SBTV_SALSA_NOX");
            return !(e && e[0] == '0');
        }();
        nox = env_nox && fft_cols_inv_step_ok(op.fp) && !crit2 && !graph_wanted(cnt) && x_out != nullptr;
        gb[1] = gb[0];
        bub[1] = bub[0];
        if (nox) {
            SBTV_TRY(ws_get_t(ctx, "salsa.bu1", cnt, &bub[1]));
            SBTV_TRY(ws_get_t(ctx, "salsa.g1", cnt, &gb[1]));
        }
        direct_last = direct_last_ok && !nox;
        // small per-image parameter arrays: [taps | mu | thr]
        const size_t nt = (size_t)batch * taille * taille;
        npar = nt + 2 * (size_t)batch;
        SBTV_TRY(ws_get_t(ctx, "salsa.par", npar, &par));
        taps_d = par;
        mu_d = par + nt;
        thr_d = mu_d + batch;
        SBTV_TRY(ws_get_t(ctx, "salsa.frozen", (size_t)batch, &frozen_d));
        nrb = fft_rows_blocks(op.fp);
        npb = fft_cols_blocks(op.fp);      // partial sums per image of the fused column/bookkeeping pass
        SBTV_TRY(ws_get_t(ctx, "salsa.acc", (size_t)batch * 3 * nrb, &acc));
        SBTV_TRY(ws_get_t(ctx, "salsa.post", (size_t)batch * 6 * npb, &postp));
        SalsaScal *scal_d = nullptr;       // [2][batch]
        SBTV_TRY(ws_get_t(ctx, "salsa.scal", 2 * (size_t)batch, &scal_d));
        SBTV_TRY(ws_get_t(ctx, "salsa.o4", (size_t)batch * 4, &o4));

        PinnedLayout lay;
        const auto f_scal = lay.add<SalsaScal>(2 * (size_t)batch);                  // scalars of an iteration, by parity
        const auto f_init = lay.add<SalsaScal>((size_t)batch);                      // initial objective (own slot)
        const auto f_psum = lay.add<double>(2 * (size_t)batch * FSTRIDE);           // prox step sums of optimistic launches
        const auto f_tags = lay.add<double>(2 * (size_t)batch * SALSA_TAGS);        // completion tags of the two slots
        const auto f_itag = lay.add<double>((size_t)batch * SALSA_TAGS);            // ... and of the initial objective
        const auto f_par = lay.add<double>(npar);                                   // parameter upload staging
        const auto f_frozen = lay.add<int>((size_t)batch);                          // frozen flags for upload
        void *ph = nullptr, *pd = nullptr;
        SBTV_TRY(pinned_get(ctx, lay.bytes(), &ph, &pd));
        scal_h = f_scal.at(ph), scal_hd = f_scal.at(pd);
        init_h = f_init.at(ph), init_hd = f_init.at(pd);
        psum_h = f_psum.at(ph), psum_hd = f_psum.at(pd);
        tags_h = f_tags.at(ph), tags_hd = f_tags.at(pd);
        init_tags_h = f_itag.at(ph), init_tags_hd = f_itag.at(pd);
        frozen_h = f_frozen.at(ph);
        for (int b = 0; b < batch; ++b) frozen_h[b] = 0;
        for (size_t i = 0; i < f_tags.count; ++i) tags_h[i] = 0.0;
        for (size_t i = 0; i < f_itag.count; ++i) init_tags_h[i] = 0.0;
        // taps, mu and the prox threshold go up through pinned memory: no synchronisation (every call ends with one)
        double *par_stage = f_par.at(ph);
        for (size_t q = 0; q < nt; ++q) par_stage[q] = taps[q];
        for (int b = 0; b < batch; ++b) {
            par_stage[nt + b] = mu[b];
            par_stage[nt + batch + b] = tau[b] / mu[b];   // threshold = tau/mu (:394)
        }
        // one small kernel reads them from the pinned block and clears the frozen flags (a memset and a copy are two blit
        // launches with 10-20 us of idle stream around each)
        hipLaunchKernelGGL(salsa_setup_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double *)f_par.at(pd), par, (int)npar,
                           frozen_d, batch);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    }

    // operator spectra: H from the taps (resize.m), Yh = fft2(y)
    int spectra() {
        // H depends on the taps and the plan only: a call with the taps of the previous call on this context (the same problem
        // solved again, a sweep over tau / mu, the exact repeat of an optimistic solve) finds it in its workspace
        const long long dims[6] = {M, N, batch, taille, op.fp.u_tiled, (long long)op.fp.u_img};
        const size_t nt = (size_t)batch * taille * taille;
        const bool same = ctx->salsa_h_ptr == (const void *)op.Hs && std::equal(dims, dims + 6, ctx->salsa_h_dims) &&
                          ctx->salsa_h_taps.size() == nt && std::equal(taps, taps + nt, ctx->salsa_h_taps.begin());
        if (!same) {
            ctx->salsa_h_ptr = nullptr;
            SBTV_TRY(psf_spectrum(ctx, op.fp, taps_d, taille, op.Hs));
            ctx->salsa_h_taps.assign(taps, taps + nt);
            std::copy(dims, dims + 6, ctx->salsa_h_dims);
            ctx->salsa_h_ptr = (const void *)op.Hs;
        }
        SBTV_TRY(op_spectrum(ctx, op.fp, yd, nullptr, op.S, op.Ys));
        h_numA.assign(batch, 0);
        h_numAt.assign(batch, 1);            // ATy = AT(y) (:288-289)
        ctx->calls += 2LL * batch;           // AT(y), invLS(ATy) size check (:298)
        return 0;
    }

    // initialisation (:366-381), then the initial objective (:399-401): resid = y - A(x).  Its scalars go to their own pinned
    // slot with completion tags and are read when the first outer iteration is processed: the loop is enqueued without
    // waiting for them.
    int start() {
        double *x = xbuf[0], *bu = bub[0], *g = gb[0];
        if (zero_start) ctx->calls += batch;                                      // AT(zeros) == 0: cleared below
        else SBTV_TRY(op_init_x(ctx, op, opts->initialization, yd, xi, x));       // ATy, or the caller's array
        // u = x ; bu = 0 ; g = x - bu = x (:392-393) ; duals zero (:418-421).  From the zero start x = u = 0, g is not read
        // before the first bookkeeping pass writes it (the first prox is not launched, see the loop), and neither start
        // clears the duals: the first prox that is launched treats them as zero (cold start flag)
        if (!zero_start) {
            SBTV_HIP(ctx, hipMemcpyAsync(u, x, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
            SBTV_HIP(ctx, hipMemcpyAsync(g, x, sizeof(double) * cnt, hipMemcpyDeviceToDevice, ctx->stream));
            SBTV_HIP(ctx, hipMemsetAsync(bu, 0, sizeof(double) * cnt, ctx->stream));
        }
        SBTV_TRY(prox_reset(ctx, pp, thr_d, 1.0, opts->TViters, opts->chambolle_tol, opts->chambolle_tau, false, nullptr));
        obj_prev.assign(batch, 0.0);
        Collect c{};
        if (zero_start) {
            // x = u = bu = 0: resid = y, TV(u) = 0, mse(1) = sum true^2 / P.  One pass clears the three images and leaves
            // the partial sums (no transform of a zero image, no separate clears)
            double *accz = nullptr, *postz = nullptr;
            int nz = 0;
            SBTV_TRY(salsa_zero_start(ctx, yd, want_mse ? td : nullptr, x, u, bu, P, batch, (double)M * (double)N, &accz, &postz,
                                      &nz));
            c = Collect{accz, nz, nullptr, 0, postz, nz, nullptr, 0, 0, 0ull, nullptr};
        } else {
            // open-coded, not op_resid: the TV partials of u are launched between the two passes of the residual
            double *tvp = nullptr;
            int ntv = 0;
            RowsArgs a{};
            a.dir_fwd = 1;
            a.op = OP_RESID;
            a.H = op.Hs;
            a.Y = op.Ys;
            a.acc = acc;
            SBTV_TRY(fft_cols_fwd(ctx, op.fp, x, nullptr, op.S));
            SBTV_TRY(tvnorm_partials(ctx, u, M, N, batch, &tvp, &ntv));
            SBTV_TRY(fft_rows(ctx, op.fp, op.S, nullptr, a));
            if (want_mse) SBTV_TRY(pair_sums(ctx, x, td, P, batch, o4));
            c = Collect{acc, nrb, tvp, ntv, nullptr, 0, nullptr, 0, 0, 0ull, want_mse ? o4 : nullptr};
        }
        hipLaunchKernelGGL(salsa_collect_kernel, dim3(7, batch), dim3(256), 0, ctx->stream, c, (ProxCtrl *)nullptr,
                           (unsigned long long)(uintptr_t)init_hd, (const int *)nullptr, 0,
                           (unsigned long long)(uintptr_t)init_tags_hd, 1.0);
        SBTV_HIP(ctx, hipGetLastError());
        ctx->calls += batch;
        return 0;
    }

    // objective(1), mses(1) from the initial objective's slot, once: waits for its tags
    int read_initial() {
        if (init_read) return 0;
        init_read = true;
        volatile const double *tg = init_tags_h;
        for (unsigned spin = 0;; ++spin) {
            bool ready = true;
            for (int b = 0; b < batch && ready; ++b)
                for (int i = 0; i < 8 && ready; ++i) ready = (tg[(size_t)b * SALSA_TAGS + i] == 1.0);
            if (ready) break;
            if (spin > 2000) {                                 // not there after a while: let the stream finish
                SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
                break;
            }
            struct timespec ts = {0, 5000};
            nanosleep(&ts, nullptr);
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        for (int b = 0; b < batch; ++b) {
            h_numA[b] += 1;
            const double f0 = 0.5 * (init_h[b].resid2 * op.parseval) + tau[b] * init_h[b].tv_u;
            obj_prev[b] = f0;
            if (objective) objective[(size_t)b * (maxiter + 1)] = f0;
            if (times) times[(size_t)b * (maxiter + 1)] = 0.0;
            if (mses && want_mse) mses[(size_t)b * (maxiter + 1)] = init_h[b].mse_num / (double)P;
        }
        return 0;
    }

    Collect make_collect(int outer, bool spec) const {
        const int slot = outer & 1;
        return Collect{acc, nrb, nullptr, 0, postp, npb, spec ? pp.partials + (size_t)slot * pp.part_stride : nullptr, pp.fnblk,
                       opts->TViters, (unsigned long long)(uintptr_t)(psum_hd + (size_t)slot * batch * FSTRIDE), nullptr};
    }
    int launch_collect(int outer, bool spec, bool tagged) {
        const int slot = outer & 1;
        const Collect c = make_collect(outer, spec);
        // the collector writes the eight scalars straight into pinned host memory (no copy kernel).  Eager launches:
        // it tags them with the iteration number (the host polls the tags); inside a captured graph the arguments are
        // frozen, so replay keeps the event
        hipLaunchKernelGGL(salsa_collect_kernel, dim3(spec ? 7 + opts->TViters : 7, batch), dim3(256), 0, ctx->stream, c, pp.ctrl,
                           (unsigned long long)(uintptr_t)(scal_hd + (size_t)slot * batch), (const int *)frozen_d, 1,
                           tagged ? (unsigned long long)(uintptr_t)(tags_hd + (size_t)slot * batch * SALSA_TAGS) : 0ull, (double)outer);
        SBTV_HIP(ctx, hipGetLastError());
        return 0;
    }
    int flush_pending() {
        if (!pend.valid) return 0;
        pend.valid = false;
        return launch_collect(pend.outer, pend.spec, true);
    }

    // enqueue the kernels of outer iteration `outer` (reads x = xbuf[(outer-1)&1] through g, writes
    // xbuf[outer&1]); eager: not inside a graph capture (tags instead of an event, the prox bracketed with events)
    int enqueue_body(int outer, bool eager) {
        static const bool piggyback = [] {
            const char *e = getenv("SBTV_COLLECT_RIDE");
            return !(e && e[0] == '0');
        }();
        const int slot = outer & 1;
        const bool tagged = eager;
        const bool spec = spec_ok && outer >= 2;
        // the prox is bracketed by events on every 32nd iteration only: an event record leaves the stream idle for
        // 5-6 us; sbtv_last_timing scales the sampled time to all iterations
        // (4, 12, 36, 68, ...: warm-started proxes; the first one launched starts cold.  Iteration 12 as well, so that a
        // 20-step call - what the driver times - rests on two samples, not one)
        const bool timed = eager && ((outer & 31) == 4 || outer == 12);
        slot_tagged[slot] = tagged;
        slot_spec[slot] = spec;
        double *xn = (direct_last && outer == maxiter) ? x_out : xbuf[slot];
        const double *xprev = xbuf[slot ^ 1];
        // the previous iteration's collector: rides on this iteration's first (optimistic) launch, or gets its own
        SideJob side{};
        if (pend.valid && spec) {
            const int ps = pend.outer & 1;
            side.c = make_collect(pend.outer, pend.spec);
            side.out_addr = (unsigned long long)(uintptr_t)(scal_hd + (size_t)ps * batch);
            side.tags_addr = (unsigned long long)(uintptr_t)(tags_hd + (size_t)ps * batch * SALSA_TAGS);
            side.frozen = frozen_d;
            side.seq = (double)pend.outer;
            side.nblocks = 7 + (pend.spec ? opts->TViters : 0);
            pend.valid = false;
        } else {
            SBTV_TRY(flush_pending());
        }
        // (1) TV prox with warm-started duals (:429); the control block was re-armed by the first (exact) iteration's
        //     collector (or by prox_reset before the loop); optimistic launches leave it alone
        if (timed) SBTV_HIP(ctx, hipEventRecord(ev_p0[slot], ctx->stream));
        // u = g - lambda div p written by the last launch.  Optimistic mode: no stop-rule kernels, no redo pass; the
        // host applies the rule over all TViters steps when it reads the iteration's scalars
        ProxPlan pps = pp;
        pps.partials = pp.partials + (size_t)slot * pp.part_stride;
        // From the zero start (INITIALIZATION 0: x = 0, bu = 0) the first prox input is g = 0: u = div p - g/lambda = 0,
        // err = 0 <= tol, so chambolle_prox_TV_stop.m:131 stops at k = 1 with p = 0 and f = 0 - everything is already
        // in place (u = 0, duals = 0) and no launch is needed; the host books the one iteration.
        // (the duals are never cleared: the first prox that is launched starts cold)
        if (!(zero_start && outer == 1))
            SBTV_TRY(prox_iterate(ctx, pps, gb[(outer - 1) & 1], opts->TViters, u, outer == (zero_start ? 2 : 1), spec,
                                  spec ? ((outer - 2) * nl_prox) & 1 : 0, side.nblocks ? &side : nullptr));
        if (timed) SBTV_HIP(ctx, hipEventRecord(ev_p1[slot], ctx->stream));
        prox_timed[slot] = timed;
        // (2) LS step in the spectral domain + residual energy (:434-444)
        RowsArgs a{};
        a.dir_fwd = 1;
        a.dir_inv = 1;
        a.op = OP_SALSA;
        a.H = op.Hs;
        a.Y = op.Ys;
        a.mu = mu_d;
        a.acc = acc;
        a.frozen = frozen_d;
        SBTV_TRY(fft_cols_fwd_f(ctx, op.fp, u, bub[(outer - 1) & 1], op.S, frozen_d));
        SBTV_TRY(fft_rows(ctx, op.fp, op.S, op.S, a));
        // (3) inverse column pass fused with the bu update, the next prox input and the sums
        //     incl. TVnorm(u) (:440-451), while x is still in registers
        ColsPost cp;
        cp.u = u;
        cp.bu = bub[outer & 1];
        cp.g = gb[outer & 1];
        if (nox) {
            cp.bu_in = bub[(outer - 1) & 1];
            cp.skip_x = 1;
        }
        cp.tru = td;
        cp.xprev = crit2 ? xprev : nullptr;
        cp.partials = postp;
        SBTV_TRY(fft_cols_inv_post(ctx, op.fp, op.S, xn, op.inv_scale, frozen_d, cp));
        // (4) the collector: deferred to the next iteration's first launch when that iteration will exist and be
        //     optimistic too (the host is then one iteration ahead anyway), else launched here
        if (spec && eager && lag == 1 && outer < maxiter && piggyback) {
            pend.valid = true;
            pend.outer = outer;
            pend.spec = spec;
            return 0;
        }
        return launch_collect(outer, spec, tagged);
    }
    // Small problems are launch-bound (about a dozen kernels of a few microseconds): from the third outer
    // iteration on, the body of each x-buffer slot is captured once and replayed with one hipGraphLaunch.
    int enqueue(int outer) {
        const int slot = outer & 1;
        hipGraphExec_t(&gexec)[2] = graphs.g;
        if (use_graph && outer >= 3) {
            if (!gexec[slot]) {
                if (graph_begin(ctx) != 0 || graph_end(ctx, enqueue_body(outer, false), &gexec[slot]) != 0) {
                    use_graph = false;                    // capture unavailable: keep launching eagerly
                    gexec[slot] = nullptr;
                }
            }
            if (gexec[slot]) {
                SBTV_HIP(ctx, hipGraphLaunch(gexec[slot], ctx->stream));
                SBTV_HIP(ctx, hipEventRecord(ev_done[slot], ctx->stream));
                return 0;
            }
        }
        return enqueue_body(outer, true);
    }

    // host side of outer iteration `outer`: traces + stopping rule (:444-482)
    int process(int outer) {
        const int slot = outer & 1;
        SBTV_TRY(read_initial());                                            // objective(1), mses(1): long there by now
        if (pend.valid && pend.outer == outer) SBTV_TRY(flush_pending());     // no later iteration took it along
        // until the collector of iteration `outer` has delivered all eight scalars (and the step sums) of every image
        if (slot_tagged[slot])
            SBTV_TRY(wait_tags(ctx, tags_h + (size_t)slot * batch * SALSA_TAGS, batch, SALSA_TAGS, 8,
                               slot_spec[slot] ? opts->TViters : 0, (double)outer));
        else SBTV_TRY(wait_event(ctx, ev_done[slot]));
        if (prox_timed[slot]) {
            float ms = 0.f;
            SBTV_HIP(ctx, hipEventSynchronize(ev_p1[slot]));
            SBTV_HIP(ctx, hipEventElapsedTime(&ms, ev_p0[slot], ev_p1[slot]));
            ms_prox += ms;
            for (int b = 0; b < batch; ++b)
                if (!frozen[b]) prox_iters_timed += slot_spec[slot] ? (long long)opts->TViters : (long long)scal_h[(size_t)slot * batch + b].pad;
            prox_timed[slot] = false;
        }
        // optimistic launches: the rule stopped a prox before its last step -> start over, exactly
        if (slot_spec[slot])
            SBTV_TRY(spec_stop_rule(ctx, pp, psum_h + (size_t)slot * batch * FSTRIDE, opts->TViters, opts->chambolle_tol,
                                    frozen.data()));
        const double tnow = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        bool changed = false;
        for (int b = 0; b < batch; ++b) {
            if (frozen[b]) continue;
            const SalsaScal &s = scal_h[(size_t)slot * batch + b];
            h_numA[b] += 1;
            h_nouter[b] = outer;
            double prox_k = s.pad;                   // exact launches: iterations booked by the stop-rule kernels
            if (zero_start && outer == 1) prox_k = 1.0;   // the prox of a zero image: one iteration, not launched
            if (slot_spec[slot]) prox_k = (double)opts->TViters;    // optimistic launches: all steps ran
            prox_iters_run += (long long)prox_k;
            ctx->calls += 2;   // invLS + A (callcounter)
            const double f = 0.5 * (s.resid2 * op.parseval) + tau[b] * s.tv_u;               // :444
            if (objective) objective[(size_t)b * (maxiter + 1) + outer] = f;
            if (mses && want_mse) mses[(size_t)b * (maxiter + 1) + outer] = s.mse_num / (double)P;   // :446-449
            if (distance) distance[(size_t)b * maxiter + (outer - 1)] = sqrt(s.dist_num) / sqrt(s.x2 + s.u2);   // :451
            if (times) times[(size_t)b * (maxiter + 1) + outer] = tnow;
            const bool stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev[b], s.dx2, s.x2, opts->tolA);
            obj_prev[b] = f;
            if (stop) {
                frozen[b] = 1;
                frozen_h[b] = 1;
                --active;
                changed = true;
            }
        }
        // park the frozen images' prox as well (optimistic launches do not re-arm the control blocks)
        if (changed && active > 0) SBTV_TRY(upload_frozen(ctx, frozen_h, frozen_d, batch, pp.ctrl));
        return 0;
    }

    // x_out: every image's x of ITS last processed iteration
    int result() {
        if (!x_out) return 0;
        for (int b = 0; b < batch; ++b) {
            double *out = x_out + (size_t)b * P;
            if (!nox) {
                // the x written by that iteration
                if (direct_last && h_nouter[b] == maxiter) continue;        // already there
                const double *src = xbuf[h_nouter[b] & 1] + (size_t)b * P;
                if (flags & SBTV_DEVICE_PTRS)
                    SBTV_HIP(ctx, hipMemcpyAsync(out, src, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
                else
                    SBTV_TRY(stage_out_copy(ctx, out, src, P, flags));        // host: through the copy lanes
                continue;
            }
            // g + bu of that iteration (x itself was never stored)
            const int par = h_nouter[b] & 1;
            const bool dev_direct = direct_last_ok;      // device-resident x_out that overlaps no input
            double *dst = dev_direct ? out : xbuf[0] + (size_t)b * P;
            const int nblk = (int)std::min<size_t>((P / 2 + 255) / 256, 2048);
            if (h_nouter[b] == 0) {          // no iteration ran (maxiter = 0): the start image
                SBTV_HIP(ctx, hipMemcpyAsync(dst, xbuf[0] + (size_t)b * P, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
            } else {
                hipLaunchKernelGGL(salsa_recover_x_kernel, dim3(nblk), dim3(256), 0, ctx->stream,
                                   (const double *)(gb[par] + (size_t)b * P), (const double *)(bub[par] + (size_t)b * P), dst, P);
                SBTV_HIP(ctx, hipGetLastError());
            }
            if (!dev_direct && (flags & SBTV_DEVICE_PTRS))
                SBTV_HIP(ctx, hipMemcpyAsync(out, dst, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
            else if (!dev_direct)
                SBTV_TRY(stage_out_copy(ctx, out, dst, P, flags));        // host: through the copy lanes
        }
        return 0;
    }

    // sbtv_last_timing and the counters, after the one synchronisation of the call
    int finish() {
        // time inside the Chambolle launches: measured on the sampled iterations, scaled to all of them
        SBTV_TRY(loop_timing(ctx, prox_iters_timed > 0 ? ms_prox * ((double)prox_iters_run / (double)prox_iters_timed) : 0.0,
                             prox_iters_run, batch, P));
        for (int b = 0; b < batch; ++b) {
            if (numA) numA[b] = h_numA[b];
            if (numAt) numAt[b] = h_numAt[b];
            if (n_outer) n_outer[b] = h_nouter[b];
        }
        return 0;
    }

    int run() {
        SBTV_TRY(open());
        SBTV_TRY(spectra());
        SBTV_TRY(start());
        frozen.assign(batch, 0);
        h_nouter.assign(batch, 0);
        active = batch;
        // The six events of the loop belong to the context (created on first use: creating and destroying them cost every
        // call ~20 us of host time before its first launch)
        for (auto &e : ctx->loop_ev)
            if (!e) SBTV_HIP(ctx, hipEventCreate(&e));
        for (int s = 0; s < 2; ++s) {
            ev_done[s] = ctx->loop_ev[s];
            ev_p0[s] = ctx->loop_ev[2 + s];
            ev_p1[s] = ctx->loop_ev[4 + s];
        }
        t0 = std::chrono::steady_clock::now();
        // Optimistic prox launches: the Chambolle launches of an outer iteration run all TViters iterations without
        // stop-rule kernels and without the redo pass (three launches less per outer iteration); the collector applies the
        // rule over all steps at the end of the iteration.  Natural images never meet err <= tol inside a prox
        // (SURVEY.md section 8 a-1); if one does, the solve is repeated from the start with exact launches (bit 1 of
        // `speculate`), so the result is always that of the exact rule.
        // The first outer iteration always runs exactly: from the zero start its prox input is flat and the rule stops at k = 1.
        spec_ok = spec_wanted && !graph_wanted(cnt) && prox_spec_ok(pp, gb[0], u, opts->TViters);
        nl_prox = prox_launches(pp, opts->TViters);
        use_graph = graph_wanted(cnt);
        int done = 0;
        SBTV_TRY(pipelined_loop(ctx, &done, maxiter, lag, true, [&](int k) { return enqueue(k); }, [&](int k) { return process(k); },
                                [&] { return active > 0; }));
        SBTV_TRY(read_initial());
        SBTV_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
        SBTV_TRY(result());
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the one synchronisation of the call
        return finish();
    }
};

}  // namespace

extern "C" int sbtv_SALSA_v2(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                             const double *tau, const double *mu, const sbtv_salsa_opts *opts, const double *true_x,
                             const double *x_init, double *x_out, double *objective, double *distance, double *times,
                             double *mses, int *numA, int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!tau || !mu) return fail(ctx, SBTV_ERR_BADARG, "SALSA_v2: missing required argument");
    // maxiter = 0 is a valid call here: no iteration runs, x_out receives the start image
    SBTV_TRY(check_common(ctx, "SALSA_v2", y, taps, opts, x_init, M, N, batch, taille, "x_init", true, false));
    for (int b = 0; b < batch; ++b)
        if (!(mu[b] > 0.0)) return fail(ctx, SBTV_ERR_MISSING_LS, "(A^T A + mu I)^(-1) must be specified: mu must be > 0");
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    // a batch: the images are independent (each stops by its own rule) -> two lanes of this context, group.hip
    if (sbtv_group *lg = lanes_group(ctx, batch, false)) {
        LaneCall lc(ctx, lg);
        return lc.done(salsa_sharded(lg, y, M, N, batch, taps, taille, tau, mu, opts, true_x, x_init, x_out, objective,
                                     distance, times, mses, numA, numAt, n_outer, flags), batch);
    }
    // start of the device-side clock of the call (sbtv_last_timing[0]): recorded while the stream is still idle - an event
    // record between two kernels would cost the stream 5-6 us
    SBTV_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    const size_t cnt = (size_t)M * N * batch;
    const double *yd = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "salsa.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "salsa.true", true_x, cnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "salsa.xinit", x_init, cnt, flags, &xi));
    // optimistic prox launches first, unless bit 1 of `speculate` asks for exact ones; repeated exactly if the rule fired
    return canary_epilogue(ctx, solve_with_exact_repeat(ctx, !(opts->speculate & 2), [&](bool spec) {
        SalsaRun r{ctx, yd, M, N, batch, taps, taille, tau, mu, opts, td, xi, x_out, objective, distance, times, mses,
                   numA, numAt, n_outer, flags, spec};
        return r.run();
    }));
}

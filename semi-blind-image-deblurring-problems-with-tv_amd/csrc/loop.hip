// Host side of the solver loops (SALSA, FISTA, C-SALSA, CoRAL; the SAPG loops use the waits and the graph replay): waits
// for the device, the stop rule of optimistic prox launches, frozen images, hipGraph replay and the loop's diagnostics.
// The pipelined loop itself and the exact repeat of a solve are templates in sbtv_internal.h.
#include <chrono>
#include <cmath>

#include <sys/resource.h>
#include <time.h>

#include "sbtv_internal.h"

namespace sbtv {

// images the host has frozen: their prox control block is parked (done = 1)
__global__ void prox_park_kernel(ProxCtrl *__restrict__ ctrl, const int *__restrict__ frozen, int batch) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch && frozen[b]) ctrl[b].done = 1;
}

int upload_frozen(sbtv_ctx *ctx, const int *frozen_h, int *frozen_d, int batch, ProxCtrl *park_ctrl) {
    SBTV_HIP(ctx, hipMemcpyAsync(frozen_d, frozen_h, sizeof(int) * batch, hipMemcpyHostToDevice, ctx->stream));
    if (park_ctrl) {
        hipLaunchKernelGGL(prox_park_kernel, dim3((batch + 63) / 64), dim3(64), 0, ctx->stream, park_ctrl,
                           (const int *)frozen_d, batch);
        SBTV_HIP(ctx, hipGetLastError());
    }
    return 0;
}

int spec_stop_rule(sbtv_ctx *ctx, ProxPlan &pp, const double *stepsums, int K, double tol, const int *frozen) {
    for (int b = 0; b < pp.batch; ++b) {
        if (frozen && frozen[b]) continue;
        const double *ps = stepsums + (size_t)b * FSTRIDE;
        for (int k = 1; k < K; ++k)
            if (!(sqrt(ps[k - 1]) > tol * SPEC_TOL_GUARD)) return SOLVE_RESTART_EXACT;
        for (int k = 1; k <= K && !pp.esub_off; ++k)
            if (!(ps[k - 1] > ESUB_MARGIN * tol * tol)) {
                pp.esub_off = 1;
                ctx->solve_stats[1] += 1;
            }
    }
    return 0;
}

int loop_timing(sbtv_ctx *ctx, double prox_ms, long long prox_iters, int batch, size_t P) {
    float ms = 0.f;
    SBTV_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->timing[0] = ms;
    ctx->timing[1] = prox_ms;
    ctx->timing[2] = (double)prox_iters / batch;
    ctx->timing[3] = 40.0 * (double)P * (double)prox_iters;
    return 0;
}

// the thread's rusage counters go into hstat as negatives at the start of a loop and the counters at its end are added
void host_stats_begin(sbtv_ctx *ctx) {
    struct rusage ru {};
    (void)getrusage(RUSAGE_THREAD, &ru);
    ctx->hstat = HostStats{};
    ctx->hstat.nvcsw = -(double)ru.ru_nvcsw;
    ctx->hstat.nivcsw = -(double)ru.ru_nivcsw;
    ctx->hstat.minflt = -(double)ru.ru_minflt;
    ctx->hstat.majflt = -(double)ru.ru_majflt;
}
void host_stats_end(sbtv_ctx *ctx) {
    struct rusage ru {};
    (void)getrusage(RUSAGE_THREAD, &ru);
    ctx->hstat.nvcsw += (double)ru.ru_nvcsw;
    ctx->hstat.nivcsw += (double)ru.ru_nivcsw;
    ctx->hstat.minflt += (double)ru.ru_minflt;
    ctx->hstat.majflt += (double)ru.ru_majflt;
}

// Polls the tags (the host is normally one iteration ahead), yielding the core between polls.  No HIP call in the normal
// case: a stream query makes the runtime append a marker packet, which costs the stream 5-6 us before the next kernel.
// Only after 50 ms without the tags is the stream asked, so that a failed launch cannot leave the host waiting.
// The wait has three phases: (1) spin on the tags for up to `spin_us` microseconds (default 150; SBTV_TAG_SPIN_US):
// an outer iteration of a small image takes 50 us and only ONE more iteration is queued behind it, while a
// nanosleep of 5 us returns after 55-60 us (the kernel's default timer slack is 50 us) or much later when the core
// went into a deep idle state - a host that sleeps there lets the queue run dry and a 512^2 solve then runs at a
// third of its speed (the "slow mode" of round 2, `sbtv_last_host_stats`); (2) sleep between polls - a 2048^2
// iteration takes 240 us, the spin would burn a core for nothing; (3) after 50 ms ask the stream.
int wait_tags(sbtv_ctx *ctx, const double *tags, int batch, int stride, int nscal, int nstep, double seq) {
    static const double spin_us = [] {
        const char *e = getenv("SBTV_TAG_SPIN_US");
        return e ? atof(e) : 150.0;
    }();
    volatile const double *tg = tags;
    const auto t_begin = std::chrono::steady_clock::now();
    auto t_query = t_begin;
    bool slept = false;
    HostStats &hs = ctx->hstat;
    hs.waits += 1;
    for (unsigned spin = 0;; ++spin) {
        bool ready = true;
        for (int b = 0; b < batch && ready; ++b) {
            for (int i = 0; i < nscal && ready; ++i) ready = (tg[(size_t)b * stride + i] == seq);
            for (int i = 0; i < nstep && ready; ++i) ready = (tg[(size_t)b * stride + 8 + i] == seq);
        }
        if (ready) {
            if (spin == 0) hs.ready_at_once += 1;
            break;
        }
        __builtin_ia32_pause();
        if ((spin & 15) != 15) continue;                       // look at the clock every 16th poll only
        const auto now = std::chrono::steady_clock::now();
        if (std::chrono::duration<double, std::micro>(now - t_begin).count() < spin_us) continue;
        struct timespec ts = {0, 5000};
        nanosleep(&ts, nullptr);
        hs.sleeps += 1;
        slept = true;
        if (now - t_query > std::chrono::milliseconds(50)) {
            hs.stream_queries += 1;
            const hipError_t e = hipStreamQuery(ctx->stream);
            if (e == hipSuccess) {
                SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));     // everything has run: the scalars are there
                break;
            }
            if (e != hipErrorNotReady) return fail_hip(ctx, e, "hipStreamQuery", __FILE__, __LINE__);
            t_query = std::chrono::steady_clock::now();
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const double w = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    hs.wait_s += w;
    if (w > hs.wait_max_s) {
        hs.wait_max_s = w;
        hs.wait_max_outer = seq;
    }
    if (slept) hs.waits_slept += 1;
    return 0;
}

// ---- host waits inside the solver loops -----------------------------------------------------------------
// One outer iteration of a small image takes tens of microseconds; a host thread that blocks in
// hipEventSynchronize / hipStreamSynchronize is woken much later than that and the GPU queue runs dry.  These
// helpers can poll (hipEventQuery / hipStreamQuery) for up to 2 ms before they fall back to the blocking call.
// Opt-in (SBTV_SPIN=1): measured on MI355X it helps at 512^2 (8 500 vs 6 500 SALSA iterations/s) and hurts at 256^2
// and 1024^2 (profiles/r02_small_sizes.md) - the polling calls compete with the launches of the same thread.
static inline bool spin_enabled() {
    static const bool on = [] {
        const char *e = getenv("SBTV_SPIN");
        return e && e[0] == '1';
    }();
    return on;
}
template <class Q>
static inline hipError_t poll_2ms(Q query) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0;; ++it) {
        const hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        if ((it & 63) == 63 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2e-3)
            return hipErrorNotReady;
    }
}
int wait_event(sbtv_ctx *ctx, hipEvent_t ev) {
    if (spin_enabled()) {
        const hipError_t e = poll_2ms([&] { return hipEventQuery(ev); });
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) return fail_hip(ctx, e, "hipEventQuery", __FILE__, __LINE__);
    }
    SBTV_HIP(ctx, hipEventSynchronize(ev));
    return 0;
}
int wait_stream(sbtv_ctx *ctx) {
    if (spin_enabled()) {
        const hipError_t e = poll_2ms([&] { return hipStreamQuery(ctx->stream); });
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) return fail_hip(ctx, e, "hipStreamQuery", __FILE__, __LINE__);
    }
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- hipGraph replay of launch-bound iteration bodies -------------------------------------------
// Small images make the solver loops latency-bound (20-odd dependent kernels of a few microseconds per
// iteration).  With SBTV_GRAPH=1 the iteration body is captured once from the stream and replayed with one
// hipGraphLaunch: the host thread then issues one call per iteration instead of ~25.  Measured on MI355X
// (512^2 demo): 0.168 vs 0.172 ms per SAPG iteration - the loop is bound by the dependent-kernel latency on
// the GPU, not by host launch cost - so replay is opt-in (it mainly frees the host core when 8 ranks share
// a node).  Results are bit-identical either way (tests/test_gpu_modes.py).
bool graph_wanted(size_t total_px) {
    static const char *e = getenv("SBTV_GRAPH");
    (void)total_px;
    return e && e[0] == '1';
}

int graph_begin(sbtv_ctx *ctx) {
    SBTV_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    return 0;
}

// Ends the capture started by graph_begin (always, so the stream leaves capture mode even when the body
// failed) and instantiates the graph.  body_rc is the status of the captured enqueue code.
int graph_end(sbtv_ctx *ctx, int body_rc, hipGraphExec_t *exec) {
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    *exec = nullptr;
    if (body_rc != 0) {
        if (g) (void)hipGraphDestroy(g);
        return body_rc;
    }
    if (e != hipSuccess || !g) return fail_hip(ctx, e, "hipStreamEndCapture", __FILE__, __LINE__);
    const hipError_t ei = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
        *exec = nullptr;
        return fail_hip(ctx, ei, "hipGraphInstantiate", __FILE__, __LINE__);
    }
    return 0;
}

}  // namespace sbtv

// Internal declarations shared by the libsbtv.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/sbtv.h"
#include "pinned_layout.h"

namespace sbtv {

constexpr int kWave = 64;  // CDNA wavefront width

// ---------------------------------------------------------------------------
// per-image control block of one TV prox (device resident)
// ---------------------------------------------------------------------------
struct ProxCtrl {
    int k;         // iterations run so far
    int done;      // 1: stop rule met -> iteration kernels return at once
    int cur;       // which dual ping-pong buffer holds the current (px,py)
    int maxiter;
    int redo;      // >0: the last fused launch over-ran the stop rule; re-run that many steps from `cur`
    int f_valid;   // 1: a fused launch already stored the final f = g - lambda div p
    double err;    // last err (chambolle_prox_TV_stop.m:128)
    double lambda;
    double tol;
    double tau;
};

// ---- stop rule of a multi-buffer optimistic prox (prox_iterate modes 2-4): shared by chambolle_mb_ctrl_kernel (tv.hip)
// and by the SAPG collector / parameter-update kernels, which can apply it on their way (sapg.hip).
// Sum of the error partials of one step by ONE wave, in the fixed order of the control kernels (lane-strided over
// chunks of 1024 tiles, then the xor tree).
__device__ __forceinline__ double mb_step_sum(const double *__restrict__ p, int nblk, int lane) {
    double acc = 0.0;
    for (int q0 = 0; q0 < nblk; q0 += 64 * 16) {
        double v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + r * 64 + lane;
            v[r] = (q < nblk) ? p[q] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc += v[r];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    return acc;
}
// cont = (k < MaxIter) & (err > tol)  (chambolle_prox_TV_stop.m:131) over the `total` step sums of a prox whose launch l
// ran base + (l < extra) steps.  Stopped at the last step: the f the last launch wrote stands (f_valid).  Stopped at an
// earlier k: `cur` = the dual buffer of the launch boundary before k, `redo` = the steps from there to k (the redo
// launch re-runs them and rewrites f).
__device__ __forceinline__ void mb_apply_rule(ProxCtrl &c, const double *tots, int total, int base, int extra) {
    int k = total;
    for (int st = 0; st < total; ++st) {
        if (!((st + 1 < total) && (sqrt(tots[st]) > c.tol))) {
            k = st + 1;
            break;
        }
    }
    c.k = k;
    c.err = sqrt(tots[k - 1]);
    c.done = 1;
    if (k == total) {
        c.redo = 0;
        c.f_valid = 1;
    } else {
        int l = 0, start = 0;
        for (;; ++l) {
            const int len = base + (l < extra ? 1 : 0);
            if (k <= start + len) break;
            start += len;
        }
        c.cur = l;                              // dual buffer at the launch boundary before k (0 = the cold start)
        c.redo = k - start;
        c.f_valid = 0;
    }
}

// Scalars one SALSA outer iteration hands back to the host (per image).
struct SalsaScal {
    double resid2;   // ||y - A x||^2 (Parseval)
    double tv_u;     // TVnorm(u)
    double mse_num;  // sum (x-true)^2
    double dist_num; // sum (x-u)^2
    double x2;       // sum x^2
    double u2;       // sum u^2
    double dx2;      // sum (x-xprev)^2  (criterion 2)
    double pad;
};

// How the host side of the most recent solver loop waited for the device (sbtv_last_host_stats)
struct HostStats {
    double waits = 0;           // waits for the scalars of an iteration
    double ready_at_once = 0;   // ... that found them at the first look
    double waits_slept = 0;     // ... that went past the spin window and slept at least once
    double sleeps = 0;          // nanosleep calls
    double stream_queries = 0;  // the 50 ms fallback: the stream was asked
    double wait_s = 0, wait_max_s = 0;         // host time inside the waits: total, longest
    double enqueue_s = 0, enqueue_max_s = 0;   // host time spent enqueueing iterations: total, longest
    double wait_max_outer = 0;  // outer iteration whose scalars the longest wait was for
    // what the operating system did to the calling thread during the loop (getrusage(RUSAGE_THREAD) deltas): a host
    // thread that is taken off its core, or that blocks in a page fault, lets the one-deep queue of a small image run dry
    double nvcsw = 0, nivcsw = 0, minflt = 0, majflt = 0;
};

struct DevBuf {
    void *p = nullptr;       // what the kernels see
    void *base = nullptr;    // what hipMalloc returned (p - guard band in canary mode, else p)
    size_t bytes = 0;        // capacity behind p
};

}  // namespace sbtv

struct sbtv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    std::string err;
    long long calls = 0;
    double timing[4] = {0, 0, 0, 0};
    sbtv::HostStats hstat;
    std::map<std::string, sbtv::DevBuf> ws;   // named device workspaces (grow-only)
    // what the tap spectrum in workspace "salsa.H" was built from (sbtv_SALSA_v2 keeps it across calls with the same taps)
    std::vector<double> salsa_h_taps;
    long long salsa_h_dims[6] = {0, 0, 0, 0, 0, 0};
    const void *salsa_h_ptr = nullptr;
    std::map<int, double2 *> twiddles;         // n -> exp(-2 pi i k / n), k < n
    std::map<int, double2 *> any_axes;         // n -> Bluestein tables of the arbitrary-size path (fft_any.inc)
    bool any_attr_done = false;                // its kernel's dynamic-LDS limit has been raised on this context's device
    void *pinned = nullptr;                    // pinned host staging for scalar read-back
    size_t pinned_bytes = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t loop_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // events of the SALSA loop (created on first use)
    int cu_count = 256;
    // SBTV_CANARY=1 (read when the context is created): every workspace gets a guard band on both sides,
    // verified at the end of each C-ABI call (canary_epilogue)
    // Host <-> device staging of large pageable arrays (ctx.hip `stage_copy`): kStageThreads copy lanes, each with its
    // own stream, two pinned chunks and an event per chunk (created on first use)
    struct StageLane {
        hipStream_t s = nullptr;
        void *pin[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
    } stage[4];
    bool stage_ready = false;
    double stage_stats[4] = {0, 0, 0, 0};     // cumulative: bytes in, seconds in, bytes out, seconds out (sbtv_diag_stage_stats)
    // cumulative (sbtv_diag_solve_stats): solves repeated with exact Chambolle launches because the stop rule fired inside
    // an optimistic prox; switches of a solve from subset error sums back to full sums (ProxPlan::esub_off)
    double solve_stats[4] = {0, 0, 0, 0};
    // Lanes: a batch of independent items (images, chains) is dealt to two internal contexts on this device, one host
    // thread and one stream each, so that the launch tails and the memory-bound passes of one half run under the
    // issue-bound Chambolle launches of the other (csrc/group.hip, `lanes_group`).  Image k is computed bit for bit as
    // without lanes (a batched call computes every image like that image alone).
    struct sbtv_group *lanes = nullptr;        // created on first use, destroyed with the context
    int lanes_mode = 0;                        // 0: independent items only (default), 1: never, 2: shared-gradient chains too
    bool is_lane = false;                      // this context IS a lane: never split again
    bool canary = false;
    bool canary_dirty = true;                  // the descriptor table below is stale
    void *canary_desc = nullptr;               // device: {lo guard, hi guard} per workspace
    int *canary_bad = nullptr;                 // device: bad bytes per workspace
    int canary_n = 0, canary_cap = 0;
};

namespace sbtv {

int fail(sbtv_ctx *ctx, int code, const std::string &msg);
int fail_hip(sbtv_ctx *ctx, hipError_t e, const char *what, const char *file, int line);
void set_global_error(const std::string &msg);

#define SBTV_HIP(ctx, expr)                                                     \
    do {                                                                        \
        hipError_t e__ = (expr);                                                \
        if (e__ != hipSuccess) return sbtv::fail_hip((ctx), e__, #expr, __FILE__, __LINE__); \
    } while (0)

#define SBTV_TRY(expr)             \
    do {                           \
        int rc__ = (expr);         \
        if (rc__ != 0) return rc__; \
    } while (0)

// grow-only named workspace on the context's device
int ws_get(sbtv_ctx *ctx, const char *name, size_t bytes, void **out);
template <typename T>
inline int ws_get_t(sbtv_ctx *ctx, const char *name, size_t count, T **out) {
    void *p = nullptr;
    int rc = ws_get(ctx, name, count * sizeof(T), &p);
    *out = static_cast<T *>(p);
    return rc;
}
int pinned_get(sbtv_ctx *ctx, size_t bytes, void **out);
// the same pinned block as the host and as the device see it
template <typename T>
inline int pinned_get(sbtv_ctx *ctx, size_t bytes, T **host, T **dev) {
    void *h = nullptr, *d = nullptr;
    SBTV_TRY(pinned_get(ctx, bytes, &h));
    SBTV_HIP(ctx, hipHostGetDevicePointer(&d, h, 0));
    *host = static_cast<T *>(h);
    *dev = static_cast<T *>(d);
    return 0;
}
// item o of an optional per-item array: p + o, and null stays null
template <class T>
inline T *off(T *p, size_t o) { return p ? p + o : p; }
// do the arrays [a, a + n) and [b, b + n) overlap (null: no)
inline bool overlaps(const double *a, const double *b, size_t n) { return a && b && a < b + n && b < a + n; }
// end of a C-ABI call: with SBTV_CANARY=1 verify every guard band (one tiny kernel + a sync), else return rc
int canary_epilogue(sbtv_ctx *ctx, int rc);
int canary_verify(sbtv_ctx *ctx, int *nbuf, int *nbad, std::string *first_bad);
int twiddle_get(sbtv_ctx *ctx, int n, const double2 **out);

inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// Stage an image argument: returns a device pointer for `p` (copying from the
// host into workspace `name` when the caller passed host pointers).
int stage_in(sbtv_ctx *ctx, const char *name, const double *p, size_t count, int flags, const double **dev);
// Output staging: device pointer to write into; stage_out copies back if host.
int stage_out_buf(sbtv_ctx *ctx, const char *name, double *p, size_t count, int flags, double **dev);
int stage_out_copy(sbtv_ctx *ctx, double *host, const double *dev, size_t count, int flags);

// 1/d for a divisor of ordinary magnitude (the spectral solve: d = |H|^2 + mu in [mu, 1 + mu]): v_rcp_f64 and one cubic
// correction r0 (1 + e + e^2), e = 1 - d r0, three FMAs, within ~1 ulp of the IEEE quotient (the IEEE division expands
// to ~20 instructions with scaling steps that such divisors never need); the form validated in the fused Chambolle kernel
__device__ __forceinline__ double fast_rcp(double d) {
    const double r = __builtin_amdgcn_rcp(d);
    const double e = __builtin_fma(-d, r, 1.0);
    return __builtin_fma(r, __builtin_fma(e, e, e), r);
}

// ---- K9: Philox4x32-10 counter-based generator + Box-Muller -> standard normals.
// counter = (pixel-pair index lo, hi, step, chain) ; key = seed.  One call yields 128 random bits =
// two 53-bit uniforms = two normals = one double2 of Z.  (Statistical parity only: MATLAB's
// randn('state',1) stream cannot be reproduced)
__device__ __forceinline__ void philox_round(unsigned &c0, unsigned &c1, unsigned &c2, unsigned &c3, unsigned k0,
                                             unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned h0 = (unsigned)(p0 >> 32), l0 = (unsigned)p0, h1 = (unsigned)(p1 >> 32), l1 = (unsigned)p1;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
}
__device__ __forceinline__ double2 philox_normal_pair(size_t q, unsigned step, unsigned chain, unsigned long long seed) {
#pragma clang fp contract(off)      // the same bits from every translation unit that draws these numbers
    unsigned c0 = (unsigned)q, c1 = (unsigned)(q >> 32), c2 = step, c3 = chain;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const unsigned long long a = ((unsigned long long)c0 << 32) | c1, bb = ((unsigned long long)c2 << 32) | c3;
    const double u1 = ((double)(a >> 11) + 0.5) * (1.0 / 9007199254740992.0);    // (0,1)
    const double u2 = ((double)(bb >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    return make_double2(r * c, r * s);
}
// one element of the MYULA step  X = | X + gam (prox - X)/lamb - gam grad/sigma2 + sqrt(2 gam) Z |
// (SAPG_algorithm_Guassian.m:80-81,161), grad = scale * v; ONE definition for the element-wise kernel (scale = 1) and for
// the epilogue of the inverse column pass, no contraction anywhere in it
__device__ __forceinline__ double myula_nocontract(double x, double p, double v, double scale, double z, double gam,
                                                   double lamb, double s2, double sq2g) {
#pragma clang fp contract(off)
    const double g = v * scale;
    return fabs(((x + gam * (p - x) / lamb) - gam * (g / s2)) + sq2g * z);
}
// ---- posterior moments of the MYULA samples (sbtv_SAPG_algorithm_moments, sbtv_myula_moments)
// Welford update of one pixel's running mean / M2 with sample number k of the accumulator (rk = 1/k): ONE definition for
// every kernel that accumulates (element-wise steps, the epilogue of the inverse column pass, the seed of iteration 1), no
// contraction anywhere in it, so every path gives the same bits.  k = 1 starts the accumulator (the buffers' previous
// contents are not read).
__device__ __forceinline__ void welford_nocontract(double &mean, double &m2, double x, int k, double rk) {
#pragma clang fp contract(off)
    if (k == 1) {
        mean = x;
        m2 = 0.0;
        return;
    }
    const double d = x - mean;
    mean = mean + d * rk;
    m2 = m2 + d * (x - mean);
}
// what a MYULA step kernel accumulates: mean / m2 [batch][P] (device).  Eager launches carry the sample number k > 0 of
// the iteration (unselected iterations launch the plain kernels); a captured graph passes k = 0 and the kernel derives it
// from the iteration counter in device memory: iteration ii = it[0] is sample (ii - first) / thin + 1 when ii >= first and
// thin divides ii - first, else nothing is accumulated.
struct MomArgs {
    double *mean, *m2;
    int k;
    const int *it;
    int first, thin;
};
__device__ __forceinline__ int mom_sample(const MomArgs &m) {
    if (m.k > 0) return m.k;
    const int ii = m.it[0];
    if (ii < m.first || (ii - m.first) % m.thin != 0) return 0;
    return (ii - m.first) / m.thin + 1;
}
// two neighbouring pixels (offset o, even) of the accumulators take the sample pair r (sample number k > 0, rk = 1/k)
__device__ __forceinline__ void moments_pair(const MomArgs &m, size_t o, double2 r, int k, double rk) {
    double2 mu = make_double2(0.0, 0.0), s = make_double2(0.0, 0.0);
    if (k > 1) {
        mu = *reinterpret_cast<const double2 *>(m.mean + o);
        s = *reinterpret_cast<const double2 *>(m.m2 + o);
    }
    welford_nocontract(mu.x, s.x, r.x, k, rk);
    welford_nocontract(mu.y, s.y, r.y, k, rk);
    *reinterpret_cast<double2 *>(m.mean + o) = mu;
    *reinterpret_cast<double2 *>(m.m2 + o) = s;
}
// a moments request of sbtv_SAPG_algorithm_moments / sbtv_myula_moments after argument checks (first resolved, >= 1)
struct MomReq {
    int first, thin, pooled;
    double *mean, *var;         // [batch or 1][P]; device pointers when dev
    long long *count;           // host, [batch or 1]; may be null
    bool dev;
    bool raw;                   // var receives M2 per chain (a lane of a pooled call: the parent pools)
};
// iterations of the accumulator: first, first + thin, ... <= last; 0 when iteration ii is not one of them
inline int mom_sample_of(const MomReq *mr, int ii) {
    if (!mr || ii < mr->first || (ii - mr->first) % mr->thin != 0) return 0;
    return (ii - mr->first) / mr->thin + 1;
}
inline long long mom_count(const MomReq &mr, int last) { return (last - mr.first) / mr.thin + 1; }
// The moments request of an entry (sampler_common.hip), every refusal SBTV_ERR_BADARG "<who>: ...".  mo null: no request,
// *selp = null, and moment outputs without options are refused; an entry whose request is not optional passes selp = null and
// has a missing one refused.  Otherwise `mean` is required, thin >= 1, and first (0: the entry's first0) lies in 1..last, the
// entry's last iteration; *sel is filled and *selp points to it.  The pooled check is the caller's: check_one_posterior, or
// its own rule.
int mom_resolve(sbtv_ctx *ctx, const char *who, const sbtv_moments_opts *mo, int first0, int last, double *mean, double *var,
                long long *count, bool dev, MomReq *sel, const MomReq **selp);
// pooled = 1 over batch > 1 chains needs chains of ONE posterior: the same y [batch][P] (dev: read back from the device),
// taps [batch][taille^2], theta and sigma2 in every chain; a null array refuses too
int check_one_posterior(sbtv_ctx *ctx, const char *who, const double *y, size_t P, const double *taps, int taille,
                        const double *theta, const double *sigma2, int batch, bool dev);
// iteration 1 (the start state) as sample 1: mean = X, m2 = 0
int moments_seed(sbtv_ctx *ctx, const double *X, double *mean, double *m2, size_t P, int batch);
// mean / m2 of `batch` chains of n samples each -> req's outputs: per chain (var = m2 / (n-1), 0 for n = 1), or pooled over
// the chains with Chan's pairwise combination in chain order 0, 1, 2, ...; raw: m2 instead of var (no pooling)
int moments_finish(sbtv_ctx *ctx, const double *mean, const double *m2, size_t P, int batch, long long n, const MomReq &req);

// where the in-kernel generator of the MYULA step takes its counters from
struct RngArgs {
    unsigned long long seed;
    unsigned step, chain0;
    const double *step_dev;     // non-null: the step counter lives in device memory (graph replay)
};

// lets the MYULA step kernel (which runs right before the cold-start prox) re-arm the prox control blocks, i.e. do
// what prox_reset does with keep_cur = false and no frozen images, and so save that launch
struct ProxArm {
    ProxCtrl *ctrl;             // [batch]; nullptr: nothing to arm
    const double *lambda;       // [batch] (device)
    int maxiter;
    double tol, tau;
    const int *frozen;          // optional per-image flag: armed as done (FISTA batches)
};

// ---- lanes (group.hip): the two-stream split of a batch inside ONE context
// the internal group to deal `n_items` independent items (shared = chains that exchange their gradients) to, or nullptr
// when the call runs on ctx itself (one item, lanes switched off, ctx is a lane, or the group cannot be created)
::sbtv_group *lanes_group(sbtv_ctx *ctx, int n_items, bool shared);
// brackets a call that was handed to the lanes: books calls / timings / the error message on the parent context
struct LaneCall {
    sbtv_ctx *ctx;
    ::sbtv_group *g;
    long long calls0[8];
    LaneCall(sbtv_ctx *c, ::sbtv_group *grp);
    int done(int rc, int n_items);
};
int salsa_sharded(::sbtv_group *g, const double *y, int M, int N, int n_items, const double *taps, int taille,
                  const double *tau, const double *mu, const sbtv_salsa_opts *opts, const double *true_x,
                  const double *x_init, double *x_out, double *objective, double *distance, double *times, double *mses,
                  int *numA, int *numAt, int *n_outer, int flags);
int sapg_sharded(::sbtv_group *g, const double *y, int M, int N, int n_items, const sbtv_sapg_opts *op,
                 const double *x0, const double *noise, double *thetas, double *ps, double *sigmas, double *logpi,
                 double *logpi_wu, double *gx, double *grads, double *eb, double *x_last, int flags,
                 const MomReq *mom = nullptr);
// sbtv_SAPG_algorithm with an optional moments request (sapg.hip)
int sapg_impl(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const sbtv_sapg_opts *op, const double *x0,
              const double *noise, double *thetas, double *ps, double *sigmas, double *logpi, double *logpi_wu, double *gx,
              double *grads, double *eb, double *x_last, sbtv_allreduce_fn reduce_fn, void *reduce_user, int flags,
              const MomReq *mom);
int fista_sharded(::sbtv_group *g, const double *b, int M, int N, int n_items, const double *taps, int taille,
                  const double *tau, double L, int prox_iters, int stopcriterion, double tolerance, int maxiters,
                  int zero_start, const double *true_x, double *x_out, double *objective, double *mses, int *n_iter,
                  int flags);
int csalsa_sharded(::sbtv_group *g, const double *y, int M, int N, int n_items, const double *taps, int taille,
                   const double *mu1, const double *mu2, const double *sigma, const double *epsilon,
                   double continuationfactor, const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                   double *x_out, double *objective, double *distance1, double *distance2, double *criterion,
                   double *times, double *mses, int *numA, int *numAt, int *n_outer, int flags);
int coral_sharded(::sbtv_group *g, const double *y, int M, int N, int n_items, const double *taps, int taille,
                  const double *tau1, const double *tau2, const double *mu1, const double *mu2, const double *mu_ls,
                  int TViters2, const sbtv_salsa_opts *opts, const double *true_x, const double *x_init, double *x_out,
                  double *objective, double *distance, double *times, double *mses, int *numA, int *numAt, int *n_outer,
                  int flags);
int masked_sharded(::sbtv_group *g, const double *y, const double *mask, int M, int N, int n_items, const double *taps,
                   int taille, const double *tau, const double *mu1, const double *mu2, const sbtv_salsa_opts *opts,
                   const double *true_x, const double *x_init, double *x_out, double *objective, double *distance,
                   double *times, double *mses, int *numA, int *numAt, int *n_outer, int flags);

// ----------------------------- host side of the solver loops (loop.hip) -----
// low-latency host waits of the solver loops (poll, then block)
int wait_event(sbtv_ctx *ctx, hipEvent_t ev);
int wait_stream(sbtv_ctx *ctx);
// waits until the completion tags [batch][stride] in pinned memory hold `seq`: scalar tags 0..nscal-1 and step-sum tags
// 8..8+nstep-1 of every image (sbtv_last_host_stats records the wait)
int wait_tags(sbtv_ctx *ctx, const double *tags, int batch, int stride, int nscal, int nstep, double seq);

// hipGraph replay of launch-bound iteration bodies
bool graph_wanted(size_t total_px);
int graph_begin(sbtv_ctx *ctx);
int graph_end(sbtv_ctx *ctx, int body_rc, hipGraphExec_t *exec);
// the captured graph execs of one call: destroyed on every return path
struct GraphExecs {
    hipGraphExec_t g[2] = {nullptr, nullptr};
    ~GraphExecs() {
        for (auto e : g)
            if (e) (void)hipGraphExecDestroy(e);
    }
};

// sbtv_last_timing of a solver loop: the device time between ctx->ev[0] and ctx->ev[1] (both complete), the time inside the
// Chambolle launches, the Chambolle iterations per image and what they move (40 bytes per pixel and iteration)
int loop_timing(sbtv_ctx *ctx, double prox_ms, long long prox_iters, int batch, size_t P);
// sbtv_last_host_stats of a solver loop: begin clears ctx->hstat, end books what the operating system did to the thread
void host_stats_begin(sbtv_ctx *ctx);
void host_stats_end(sbtv_ctx *ctx);

// The pipelined host loop of the solvers: iterations *done + 1 .. maxiter, at most 1 + lag of them enqueued, processed in
// order.  It stops after maxiter, when active() turns false, or when enqueue / process return non-zero (an error, or
// SOLVE_RESTART_EXACT from spec_stop_rule); the stream is then drained.  *done: the last iteration processed.  stats: the
// loop keeps sbtv_last_host_stats (enqueue times here, waits in wait_tags).
template <class Enqueue, class Process, class Active>
int pipelined_loop(sbtv_ctx *ctx, int *done, int maxiter, int lag, bool stats, Enqueue &&enqueue, Process &&process,
                   Active &&active) {
    if (stats) host_stats_begin(ctx);
    int rc = 0, enq = *done;
    while (rc == 0 && active() && *done < maxiter) {
        while (rc == 0 && enq < maxiter && enq - *done <= lag) {
            const auto te = std::chrono::steady_clock::now();
            rc = enqueue(++enq);
            const double d = std::chrono::duration<double>(std::chrono::steady_clock::now() - te).count();
            if (stats) {
                ctx->hstat.enqueue_s += d;
                if (d > ctx->hstat.enqueue_max_s) ctx->hstat.enqueue_max_s = d;
            }
        }
        if (rc == 0) rc = process(++*done);
    }
    if (rc != 0) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    if (stats) host_stats_end(ctx);
    return 0;
}

// ----------------------------- TV kernels (tv.hip) --------------------------
struct ProxPlan {
    int M, N, batch;
    int tiles_i, tiles_j, nblk;   // blocks per image (one-iteration kernels)
    int ftiles_i, ftiles_j, fnblk; // blocks per image (temporally fused kernel)
    int cj, nw, minw, rpl;        // fused-kernel variant of this plan (columns per wave, waves, waves/SIMD, rows per lane)
    ProxCtrl *ctrl;               // [batch]
    double *pbuf;                 // [pairs][2 (px,py)][batch][M*N]; pairs = 2 (ping-pong) unless prox_reserve_pairs() asked for more
    int pairs;
    std::string tag;              // workspace name prefix
    double *partials;             // [2 sets][batch][FSTRIDE][fnblk] (or [batch][nblk] for the one-iteration kernels)
    size_t part_stride;           // doubles per set
    unsigned *counters;           // [batch] arrival tickets (in-kernel stop-rule path)
    const int *order;             // [fnblk] workgroup -> tile of the 128-row tile kernel (null: the arithmetic XCD-chunk order)
    // optimistic launches (prox_iterate spec == 1) sum their error terms over a subset of the pixels (a lower bound of the
    // step sums: enough to PROVE that the stop rule cannot have fired, tv_fused.inc ESUB).  A solver loop sets this to 1 once
    // the step sums it reads come within ESUB_MARGIN of tol^2: from then on its launches sum every pixel again, so that a
    // solve whose prox converges does not take the exact path because of the looser bound
    int esub_off;
};
int prox_plan(sbtv_ctx *ctx, int M, int N, int batch, ProxPlan *plan, const char *tag = "prox");
// (Re)initialise the control blocks: k=0, done=0 and the per-image lambda from a
// DEVICE array `lambda_dev` scaled by `lambda_scale`; keep_cur keeps the
// ping-pong index (warm start from the duals of the previous call).
int prox_reset(sbtv_ctx *ctx, const ProxPlan &pl, const double *lambda_dev, double lambda_scale,
               int maxiter, double tol, double tau, bool keep_cur, const int *frozen);
int prox_zero_duals(sbtv_ctx *ctx, const ProxPlan &pl);
int prox_set_duals(sbtv_ctx *ctx, const ProxPlan &pl, const double *px, const double *py);   // device ptrs
int prox_get_duals(sbtv_ctx *ctx, const ProxPlan &pl, double *px, double *py);               // device ptrs
// Run up to `maxiter` iterations (device-side early exit), no host sync.
// If f_out is given it receives f = g - lambda div p (fused into the last launch where possible).
// cold = true: start from px = py = 0 without reading (or requiring the caller to clear) the dual buffer; the
// control block must have been reset with keep_cur = false.
constexpr int FSMAX = 10;     // most iterations any fused Chambolle kernel runs per LAUNCH
// The after-the-fact check of an optimistic prox compares step sums that were added up in another order than the exact
// launches' (and, with ESUB, over a subset of the pixels) with tol: a sum within this relative band above tol counts as
// "fired" too and takes the exact path, so that the certificate "the rule did not fire" holds in floating point as well
constexpr double SPEC_TOL_GUARD = 1.0 + 1e-12;
constexpr double ESUB_MARGIN = 32.0;    // see ProxPlan::esub_off (step sums move by a few per cent per outer iteration, the host is one behind)
constexpr int FSTRIDE = 32;   // step slots of the error partials [batch][FSTRIDE][nblk]: most iterations of an optimistic prox
// ---- SALSA collector: what it reduces (salsa.hip launches it; the Chambolle kernels can host its blocks, tv_fused.inc)
constexpr int SALSA_TAGS = 8 + FSTRIDE;   // completion tags per image: 8 scalars + FSTRIDE prox step sums
struct Collect {
    const double *acc;      // rows kernel partials: [batch][3][nrb]           -> resid2
    int nrb;
    const double *tvp;      // tvnorm partials [batch][ntv] (initial objective) or null -> post slot 5
    int ntv;
    const double *post;     // post kernel partials [batch][6][npb]
    int npb;
    // optimistic prox launches: error partials [batch][FSTRIDE][pnblk] of the psteps iterations the launches ran
    // without a stop rule (null: the prox ran exactly); blocks 7.. total one step each for the host's rule
    const double *ppart;
    int pnblk, psteps;
    unsigned long long psum_addr;   // [batch][FSTRIDE] step sums (pinned host memory, as an integer like `out`)
    const double *mse0;     // initial objective only: pair_sums output [batch][4], element 0 -> mse_num (else null)
};
// A collector that rides on another kernel's launch: the first `nblocks` workgroups of that grid run its blocks
// (a launch costs ~5 us however little it does; these blocks finish long before the host kernel's own work)
struct SideJob {
    Collect c;
    unsigned long long out_addr, tags_addr;
    const int *frozen;
    double seq;
    int nblocks;            // 0: no side job
};
#ifdef __HIPCC__
#include "collect.inc"
#endif

int prox_iterate(sbtv_ctx *ctx, const ProxPlan &pl, const double *g, int maxiter, double *f_out = nullptr,
                 bool cold = false, int spec = 0, int spec_parity = 0, const SideJob *side = nullptr);
int prox_reserve_pairs(sbtv_ctx *ctx, ProxPlan *pl, int pairs);
int prox_launches(const ProxPlan &pl, int maxiter);
bool prox_spec_ok(const ProxPlan &pl, const double *g, const double *f_out, int maxiter);
// defaults of chambolle_prox_TV_stop.m:77-78, which FISTA, MYULA and SAPG call without options
constexpr double CHAMBOLLE_TOL = 1e-3, CHAMBOLLE_TAU = 0.249;

// ---- optimistic prox launches in the solver loops (loop.hip)
// internal status: the Chambolle stop rule fired inside an optimistic prox, the solve has to be repeated exactly
constexpr int SOLVE_RESTART_EXACT = 12345;
// cont = (k < MaxIter) & (err > tol)  (chambolle_prox_TV_stop.m:131) over the K step sums [pp.batch][FSTRIDE] of an
// optimistic prox on plan pp (images with frozen[b] set are skipped): SOLVE_RESTART_EXACT when it stopped an image before
// the last step.  Otherwise the plan's launches go back to the full error sums once the (lower-bound) subset sums come
// within ESUB_MARGIN of tol^2 (ProxPlan::esub_off, counted in solve_stats[1]).
int spec_stop_rule(sbtv_ctx *ctx, ProxPlan &pp, const double *stepsums, int K, double tol, const int *frozen = nullptr);
// Runs body(spec) - optimistic prox launches when spec - and, should it return SOLVE_RESTART_EXACT, rewinds the call
// counter, counts the repeat (solve_stats[0]) and runs body(false) with exact launches: the result is always that of the
// exact rule.
template <class Body>
int solve_with_exact_repeat(sbtv_ctx *ctx, bool spec, Body &&body) {
    const long long calls0 = ctx->calls;
    const int rc = body(spec);
    if (rc != SOLVE_RESTART_EXACT) return rc;
    ctx->calls = calls0;
    ctx->solve_stats[0] += 1;
    return body(false);
}
// images the host has frozen: their flags go up from (pinned) frozen_h to frozen_d, then the prox control blocks of
// park_ctrl (null: none) are parked (done = 1)
int upload_frozen(sbtv_ctx *ctx, const int *frozen_h, int *frozen_d, int batch, ProxCtrl *park_ctrl);
// f = g - lambda * div(p)
int prox_finish(sbtv_ctx *ctx, const ProxPlan &pl, const double *g, double *f);
// periodic TV norm of x -> out_dev[batch] (device)
int tvnorm_dev(sbtv_ctx *ctx, const double *x, int M, int N, int batch, double *out_dev);
// same without the final reduction: per-block partials [batch][nblk] (workspace owned)
int tvnorm_partials(sbtv_ctx *ctx, const double *x, int M, int N, int batch, double **partials, int *nblk);

// ----------------------------- FFT / operator (fft.hip) ---------------------
enum SpecOp {
    OP_NONE = 0,      // plain transform
    OP_MUL_H = 1,     // X *= H
    OP_MUL_HC = 2,    // X *= conj(H)
    OP_INVLS = 3,     // X /= (|H|^2 + mu)
    OP_SALSA = 4,     // X = (conj(H) Y + mu S) / (|H|^2+mu);  acc += w |Y - H X|^2
    OP_RESID = 5,     // acc += w |H X - Y|^2 (no write)
    OP_GRAD = 6,      // X = conj(H) (H X - Y) ; acc0 += w|HX-Y|^2 ; acc1/2 += w Re(D1/2 X conj(HX-Y))
    OP_ATA = 7,       // X *= |H|^2
    OP_GRADF = 8,     // X = conj(H) (H X - Y) ; acc0 += w|HX-Y|^2
    OP_CSALSA = 9,    // C-SALSA with its constraint state kept as a spectrum E (admm.hip): W = cs[0] Y + cs[1] E;
                      // X = (conj(H) W + mu S) / (|H|^2+mu); T = H X - Y; E' = T + cs[2] E (stored in place);
                      // acc0 += w|T|^2; acc1 += w|E'|^2; acc2 += w|E' - E|^2
};
struct FftPlan {
    int M, N, batch;
    int n1;                 // M/2  (column transform length, complex)
    int wave;               // 1: wave-granular kernels + tiled spectrum layout (fft_wave.inc), chosen by the image size
    int u_tiled;            // = wave: operator spectra tiled like S, U[(l/4)][k][l%4], k = 0..M/2 (else column-major U[l][k])
    size_t u_img;           // complex elements of ONE operator spectrum (H, Y, D1, D2) per image
    size_t s_img;           // complex elements of the spectrum S of one image (M/2 x N packed; M x N in generic mode)
    int generic;            // 1: arbitrary-size path (fft_any.inc): full complex spectra, n1 = M
    const double2 *tw_n1;   // twiddles of length n1
    const double2 *tw_M;    // twiddles of length M (split step)
    const double2 *tw_N;    // twiddles of length N
};
int fft_plan(sbtv_ctx *ctx, int M, int N, int batch, FftPlan *plan);
// real M x N (x batch) -> packed half spectrum S (M/2 x N complex), column pass only + row pass
// `add` (optional) is added to `x` on load (x + add).
int fft_cols_fwd(sbtv_ctx *ctx, const FftPlan &pl, const double *x, const double *add, double2 *S);
int fft_cols_inv(sbtv_ctx *ctx, const FftPlan &pl, const double2 *S, double *x, double scale);
// inverse column pass fused with the SALSA bookkeeping pass (bu, g, reductions, TV(u)); see fft.hip
struct ColsPost {
    const double *u = nullptr;
    double *bu = nullptr;
    double *g = nullptr;
    // wave-granular kernel only (sizes of fft_cols_inv_step_ok): bu is READ from bu_in (null: from `bu`, in place) and
    // written to `bu`; skip_x: the transform's output x is used for the bookkeeping but not stored (the SALSA loop can
    // recover its final x as g + bu, see salsa.hip)
    const double *bu_in = nullptr;
    int skip_x = 0;
    const double *tru = nullptr;
    const double *xprev = nullptr;
    double *partials = nullptr;      // [batch][6][fft_cols_blocks]
    // gradient-step mode (fft_cols_inv_step): ystep <- ystep - alpha * x, x itself is not stored
    double *ystep = nullptr;
    double alpha = 0.0;
    // MYULA mode (fft_cols_inv_myula): the transform's output is the gradient AT(AX - y); the chain state X = ystep is
    // advanced in place (SAPG_algorithm_Guassian.m:80-81,161), the gradient is not stored
    const double *mprox = nullptr, *msig2 = nullptr, *mZ = nullptr;
    double mgam = 0.0, mlamb = 0.0, msq2g = 0.0;
    RngArgs mrng = {0ull, 0u, 0u, nullptr};
    ProxArm marm = {nullptr, nullptr, 0, 0.0, 0.0, nullptr};
    MomArgs mom = {nullptr, nullptr, 0, nullptr, 1, 1};   // MYULA mode with moments (PM bit 128)
};
// X <- | X + gam (prox - X)/lamb - gam (scale colIFFT(S))/sigma2 + sqrt(2 gam) Z |  with the gradient still in the
// registers of the inverse column pass (same bits as fft_cols_inv followed by myula_step); Z: injected noise or null
// (then the Philox generator, `rng`); `arm` re-arms the control blocks of the cold prox that follows, as myula_step
// does.  Sizes of the wave-granular column pass only (fft_cols_inv_step_ok).
int fft_cols_inv_myula(sbtv_ctx *ctx, const FftPlan &pl, const double2 *S, double scale, double *X, const double *prox,
                       const double *Z, const double *sigma2_dev, double gam, double lamb, const RngArgs *rng,
                       const ProxArm *arm, const MomArgs *mom = nullptr);
int fft_cols_blocks(const FftPlan &pl);
// y <- y - alpha * (scale * colIFFT(S)) with the transform's output still in registers (my_fista.m:25: the gradient is
// never written); only for the sizes of the wave-granular column pass (fft_cols_inv_step_ok), same bits as
// fft_cols_inv_f followed by axpy
bool fft_cols_inv_step_ok(const FftPlan &pl);
int fft_cols_inv_step(sbtv_ctx *ctx, const FftPlan &pl, const double2 *S, double *y, double scale, double alpha,
                      const int *frozen);
// x = scale * colIFFT(S) and g = x - b from the column still in registers (sizes of fft_cols_inv_step_ok)
int fft_cols_inv_sub(sbtv_ctx *ctx, const FftPlan &pl, const double2 *S, double *x, double scale, const double *b, double *g);
int fft_cols_inv_post(sbtv_ctx *ctx, const FftPlan &pl, const double2 *S, double *x, double scale, const int *frozen,
                      const ColsPost &post);
struct RowsArgs {
    int dir_fwd;            // 1: apply forward row FFT first
    int dir_inv;            // 1: apply inverse row FFT last
    int op;                 // SpecOp
    const double2 *H;       // (M/2+1) x N per image (unpacked rows 0..M/2)
    const double2 *Y;       // same layout (OP_SALSA / OP_RESID / OP_GRAD)
    const double2 *D1, *D2; // derivative spectra (OP_GRAD), may be null
    double2 *E;             // OP_CSALSA: state spectrum, layout of H, read and written in place
    const double *cs;       // OP_CSALSA: three coefficients (device), see SpecOp
    const double *mu;       // per image (device)
    double *acc;            // partial sums [batch][3][nblk_rows]
    const int *frozen;      // optional per-image flag: skip image when set
    int shared_spec;        // 1: one spectrum set shared by the whole batch (parallel chains on one image)
};
int fft_rows(sbtv_ctx *ctx, const FftPlan &pl, const double2 *Sin, double2 *Sout, const RowsArgs &a);
int fft_rows_blocks(const FftPlan &pl);   // number of row blocks per image (acc stride)
bool fft_rows_csalsa_ok(const FftPlan &pl);   // OP_CSALSA exists in the row kernels this plan uses
// unpack packed spectrum S -> full rows 0..M/2 layout ((M/2+1) x N)
int spec_unpack(sbtv_ctx *ctx, const FftPlan &pl, const double2 *S, double2 *U);
// direct evaluation of the tap spectrum: U[(M/2+1) x N] per image from taps[batch][taille^2] (device)
int psf_spectrum(sbtv_ctx *ctx, const FftPlan &pl, const double *taps_dev, int taille, double2 *U);
int psf_spectrum_sets(sbtv_ctx *ctx, const FftPlan &pl, const double *const *taps_dev, int taille, double2 *const *U, int nsets);

// ----------------------------- elementwise (elementwise.hip) ----------------
// generic deterministic final reduction: out[b*nout + q] = sum_i partials[(b*nout+q)*n + i]
int reduce_partials(sbtv_ctx *ctx, const double *partials, int nvec, int n, double *out);
// up to four such reductions in one launch: dst[q][v] = sum_i src[q][v*n[q] + i], v < nvec[q] (unused jobs: nvec = 0)
struct RedJobs {
    const double *src[4] = {nullptr, nullptr, nullptr, nullptr};
    double *dst[4] = {nullptr, nullptr, nullptr, nullptr};
    int nvec[4] = {0, 0, 0, 0};
    int n[4] = {0, 0, 0, 0};
    int dropped = 0;               // jobs that found all four slots taken: reduce_jobs refuses such a set
    void add(const double *s, int nv, int nn, double *d) {
        for (int q = 0; q < 4; ++q)
            if (nvec[q] == 0) {
                src[q] = s;
                dst[q] = d;
                nvec[q] = nv;
                n[q] = nn;
                return;
            }
        ++dropped;
    }
};
int reduce_jobs(sbtv_ctx *ctx, const RedJobs &jb);
int ew_blocks(size_t P);
// out4_dev[b*4 + {0,1,2,3}] = sum (a-c)^2, sum a^2, sum c^2, max a
int pair_sums(sbtv_ctx *ctx, const double *a, const double *c, size_t P, int batch, double *out4_dev);
int salsa_zero_start(sbtv_ctx *ctx, const double *y, const double *tru, double *x, double *u, double *bu, size_t P, int batch,
                     double scale, double **accp, double **postp, int *nblk);
int axpy(sbtv_ctx *ctx, double *y, const double *gr, double a, size_t Ptot, const ProxArm *arm = nullptr, int batch = 0);
int fista_momentum(sbtv_ctx *ctx, const double *x, const double *xold, double *y, const double *tru, double coef,
                   double *partials, size_t P, int batch, const int *frozen);
// Z == nullptr: the normals are drawn in the kernel from `rng` (the numbers randn_kernel would have stored)
int myula_step(sbtv_ctx *ctx, double *X, const double *prox, const double *grad, const double *Z,
               const double *sigma2_dev, double gam, double lamb, size_t P, int batch, const RngArgs *rng = nullptr,
               const ProxArm *arm = nullptr, const MomArgs *mom = nullptr);
int myula_plain_step(sbtv_ctx *ctx, double *X, const double *prox, const double *grad, const double *Z,
                     const double *sigma2_dev, double gam, double lamb, size_t P, int batch, const RngArgs *rng,
                     const ProxArm *arm, const MomArgs *mom = nullptr);
int fft_cols_fwd_f(sbtv_ctx *ctx, const FftPlan &pl, const double *x, const double *add, double2 *S, const int *frozen,
                   double *tvp = nullptr);
bool fft_cols_tv_ok(const FftPlan &pl);
int fft_cols_inv_f(sbtv_ctx *ctx, const FftPlan &pl, const double2 *S, double *x, double scale, const int *frozen);

// ----------------------------- blur-operator layer of the drivers (operator.hip) ---------
// What a solve shares about its operator A = ifft2(H . fft2): the plan of `batch` images of P pixels, the packed work
// spectrum S, the spectra of the PSF (Hs, filled by the caller: psf_spectrum) and of the observation (Ys), the scale of
// the inverse column pass and the Parseval factor of the residual sums.
struct BlurOp {
    FftPlan fp;
    int batch;
    size_t P;
    double2 *S, *Hs, *Ys;
    double inv_scale, parseval;
};
// plan + the workspaces "<prefix>.S", "<prefix>.H" and "<prefix>.<y_name>" (y_name null: no observation spectrum)
int op_open(sbtv_ctx *ctx, const char *prefix, int M, int N, int batch, const char *y_name, BlurOp *op);
// U = fft2(in + add) in the layout of H, by way of the packed spectrum S (any plan: SAPG has one per spectrum set)
int op_spectrum(sbtv_ctx *ctx, const FftPlan &fp, const double *in, const double *add, double2 *S, double2 *U);
// out = real(ifft2(op(H) .* fft2(in))): OP_MUL_H, OP_MUL_HC, OP_ATA, and OP_INVLS with mu (device, per image)
int op_apply(sbtv_ctx *ctx, const BlurOp &c, int op, const double *in, double *out, const double *mu = nullptr);
// out = real(ifft2((conj(H) Y + mu fft2(in + add)) / (|H|^2 + mu))), the row pass OP_SALSA (mu: device); its residual sum
// against Y goes to acc, and c.S is left holding N times the column transform of `out`
int op_solve(sbtv_ctx *ctx, const BlurOp &c, const double *in, const double *add, const double2 *Y, const double *mu,
             double *acc, double *out);
// acc = the partial sums of ||H fft2(x) - Ys||^2 (OP_RESID: nothing is stored); images with frozen[b] set are skipped;
// tvp: the TV partials of x ride on the forward column pass (sizes of fft_cols_tv_ok)
int op_resid(sbtv_ctx *ctx, const BlurOp &c, const double *x, double *acc, const int *frozen = nullptr, double *tvp = nullptr);
// grad = AT(A x - y) (OP_GRADF), ||A x - y||^2 partial sums to acc
int op_gradf(sbtv_ctx *ctx, const BlurOp &c, const double *x, double *acc, double *grad);
// the start image by `initialization` of sbtv_salsa_opts: 0 zeros, 2 AT(y), else the caller's xi
int op_init_x(sbtv_ctx *ctx, const BlurOp &c, int initialization, const double *yd, const double *xi, double *x);

// ----------------------------- what the TV sampler drivers share on the host (sampler_common.hip) ---------
// The normals of one step as the kernels read them: the staging buffer Z of one step of host noise (null: none needed), the
// caller's device array, or null (Philox).  stage() enqueues the copy of the step's normals into Z, ptr() is what a kernel
// launched after it reads; get() is both.
struct NoiseFeed {
    sbtv_ctx *ctx;
    const double *noise;
    double *Z;
    size_t cnt;
    int stage(size_t step) const {
        if (Z) SBTV_HIP(ctx, hipMemcpyAsync(Z, noise + step * cnt, sizeof(double) * cnt, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    const double *ptr(size_t step) const { return Z ? Z : (noise ? noise + step * cnt : nullptr); }
    int get(size_t step, const double **zd) const {
        SBTV_TRY(stage(step));
        *zd = ptr(step);
        return 0;
    }
};
// The plain MYULA chain (SALSA/myula.m:13-16) on buffers its caller has set up: for ii = 2..samples - 1 the cold prox of X,
// the caller's gradient() of the likelihood at X into `grad` (times sigma2), the step; sample ii joins the moments where mom
// selects it.  sync_every > 0: the stream is synchronised every so many iterations.
struct MyulaLoop {
    double *X, *prox, *grad;
    const double *sig_d;        // [batch] (device)
    const ProxPlan *pp;
    ProxArm arm;
    NoiseFeed nz;
    double gamma, lambda;
    size_t P;
    int batch, samples, chambolleit;
    unsigned long long seed;
    int chain_offset;
    const MomReq *mom;
    double *pm_mean, *pm_m2;
    int sync_every;
};
int myula_plain_loop(sbtv_ctx *ctx, const MyulaLoop &a, const std::function<int()> &gradient);

// The front and back end of the SAPG drivers of the TV model (sapg.hip, sapg_skrock.hip, sapg_masked.hip); SapgConst, SapgChain
// and the trace layout are sapg_step.inc's.
struct SapgConst;
struct SapgChain;
// what sbtv_SAPG_algorithm refuses, with its codes; every message starts "<who>: "
int sapg_refuse(sbtv_ctx *ctx, const char *who, const double *y, int M, int N, int batch, const sbtv_sapg_opts *op);
// the constants of the parameter step; shared: one spectrum set for all chains; parseval: the factor on the collector's sums
void sapg_fill_const(SapgConst *u, const sbtv_sapg_opts *op, int M, int N, int batch, bool shared, double parseval);
// the state every chain starts from, with the burn-in sums at burnIn = 1
SapgChain sapg_chain_start(const SapgConst &u, const sbtv_sapg_opts *op);
// the start of a call whose chains own their parameters: `batch` chains at sapg_chain_start, and the block the device's `par`
// starts from: the host's taps and derivative taps of p_init for every chain, [taps | d0 | d1], then lam[batch], sigma2[batch]
int sapg_start(sbtv_ctx *ctx, const char *who, const SapgConst &u, const sbtv_sapg_opts *op, std::vector<SapgChain> *chain,
               std::vector<double> *par);
// the device side of such a call in the workspaces "<prefix>.par", ".scal" [4*batch], ".delta" [samples + 1], ".chain" and
// ".traces": par, delta(ii) and the chains uploaded, the traces zeroed; returns after the uploads have completed
struct SapgDevBufs {
    double *par, *scal, *delta, *traces;
    SapgChain *chain;
};
int sapg_device_setup(sbtv_ctx *ctx, const char *prefix, const SapgConst &u, const sbtv_sapg_opts *op,
                      const std::vector<SapgChain> &chain, const std::vector<double> &par, SapgDevBufs *d);
// enqueues the copies of the device traces and chains to the host (tr is sized here); the caller synchronises
int sapg_download(sbtv_ctx *ctx, const SapgConst &u, const SapgDevBufs &d, std::vector<double> *tr,
                  std::vector<SapgChain> *chain);
// spectra of the taps and of their parameter derivatives in `par`, ONE launch for the two or three sets (fp: u.nspec images)
int sapg_spectra(sbtv_ctx *ctx, const FftPlan &fp, const SapgConst &u, const double *par, double2 *Hs, double2 *D1s,
                 double2 *D2s);
// the traces (layout of sapg_traces, on the host) and the chains' end state -> the caller's arrays, each optional: slot 0 of
// theta / sigma2 / p is the start value, eb the four EB means (:258-284); logpi0 non-null: logpi of slot 0 per chain
struct SapgOut {
    double *thetas, *ps, *sigmas, *logpi, *logpi_wu, *gx, *grads, *eb;
};
void sapg_copy_out(const SapgConst &u, const sbtv_sapg_opts *op, const double *tr, const SapgChain *chain,
                   const double *logpi0, const SapgOut &out);

// ---- argument checks the entry points share
int check_psf_fits(sbtv_ctx *ctx, int taille, int M, int N);       // SBTV_ERR_PSF "Mask does not fit inside array"
int check_even_pixels(sbtv_ctx *ctx, int M, int N);                // SBTV_ERR_SIZE: the element-wise passes move two per lane
// x_init_name: what the caller's start array is called in its message; tv: the entry point runs a TV prox of TViters
// iterations; maxiter_positive = false: maxiter = 0 is a valid call (sbtv_SALSA_v2 returns the start image)
int check_common(sbtv_ctx *ctx, const char *who, const double *y, const double *taps, const sbtv_salsa_opts *opts,
                 const double *x_init, int M, int N, int batch, int taille, const char *x_init_name = "x_init", bool tv = true,
                 bool maxiter_positive = true);
// The stop rule of SALSA_v2.m:453-472 (CoRAL_v2.m:435-453 is the same rule), from the second iteration on: the relative
// change of the objective f (criterion 1), ||x - xprev|| / ||x|| from their squares num and den (2), f itself (3)
inline bool salsa_stop(int stopcriterion, int outer, double f, double obj_prev, double num, double den, double tolA) {
    if (outer <= 1) return false;                                        // :453
    double crit;
    if (stopcriterion == 1)
        crit = fabs(f - obj_prev) / obj_prev;                            // :456
    else if (stopcriterion == 2)
        crit = fabs(sqrt(num) / sqrt(den));                              // :460
    else
        crit = f;                                                        // :464
    return crit < tolA;                                                  // :472
}

// ----------------------------- redundant wavelet frame (wavelet.hip) ---------
// one checked transform: image size, filter length K, J = levels - 1 decomposition steps, h0 / sqrt 2 and h1 / sqrt 2
struct WavPlan {
    int M, N, K, J;
    double f0[8], f1[8];
    int bands() const { return 3 * J + 1; }
};
// argument checks of the transforms (host only, before any GPU work); orthonormal: also those of the solver
int wav_plan(sbtv_ctx *ctx, int M, int N, const double *h, int hlen, int levels, bool orthonormal, WavPlan *pl);
// z[batch][3J+1][M N] = W' x (mrdwt_TI2D) and x[batch][M N] = W z (mirdwt_TI2D), device pointers, no sync
int wav_analysis(sbtv_ctx *ctx, const WavPlan &pl, const double *x, double *z, int batch);
int wav_synthesis(sbtv_ctx *ctx, const WavPlan &pl, const double *z, double *x, int batch);
// the same synthesis; mom non-null with k > 0: every pixel of x is also sample k of the running mean / M2 mom->mean /
// mom->m2 [batch][M N], accumulated by the level-1 launch on the value it stores (wav_synthesis_moments_kernel).  x holds
// the same bits either way.
int wav_synthesis(sbtv_ctx *ctx, const WavPlan &pl, const double *z, double *x, int batch, const MomArgs *mom);
// soft(x, T) = sign(x) max(|x| - T, 0)  (SALSA/soft.m); T = 0 passes x through
__device__ __forceinline__ double wav_soft(double x, double T) { return copysign(fmax(fabs(x) - T, 0.0), x); }
// one coefficient of the MYULA step on the frame coefficients (SAPG_algorithm_1.m:133,174 with proxG = soft):
//     x + gam (soft(x, T) - x) / lamb - gam g / s2 + sqrt(2 gam) z,   T = lamb theta
// the element of wav_step_kernel (wavelet_chain.hip), no contraction anywhere in it
__device__ __forceinline__ double wav_myula_nocontract(double x, double g, double z, double T, double gam, double lamb,
                                                       double s2, double sq2g) {
#pragma clang fp contract(off)
    return ((x + gam * (wav_soft(x, T) - x) / lamb) - gam * (g / s2)) + sq2g * z;
}
// the element-wise passes over the coefficients (wavelet_chain.hip) and the per-chain kernels of the three chain drivers
// (update and trace kernels of wavelet_sapg.hip, wavelet_myula.hip, wavelet_sapg_sb.hip): WAV_EWB lanes per workgroup; an
// element-wise pass has at most WAV_EW_MAXBLK workgroups (= partial sums) per chain, a grid-stride loop beyond
constexpr int WAV_EWB = 256;
constexpr int WAV_EW_MAXBLK = 2048;
inline int wav_ew_blocks(size_t dimX) {
    const size_t nb = (dimX / 2 + WAV_EWB - 1) / WAV_EWB;
    return nb > (size_t)WAV_EW_MAXBLK ? WAV_EW_MAXBLK : (nb < 1 ? 1 : (int)nb);
}
__device__ __forceinline__ double wav_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// sum over a workgroup of WAV_EWB lanes in a fixed order (lanes, then the four waves); every lane returns the total
__device__ __forceinline__ double wav_block_sum(double v, double *red) {
    v = wav_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// The theta step of SALSA/SAPG_algorithm_1.m for the update kernels of wavelet_sapg.hip and wavelet_sapg_sb.hip, which
// store the result into their own traces.  eta / th_cur: eta(ii-1), theta(ii-1); g = ||X(ii)||_1; sum_eta over n_eta terms:
// the running sum of eta(burnIn:ii-1), which eta(ii) joins when burn (ii >= burnIn).
struct WavThetaStep {
    double eta, th;         // eta(ii), theta(ii)
    double sum_eta, n_eta;  // the running sum with eta(ii)
    double tol, mean;       // tol_thetas(ii); exp(mean(eta(burnIn:ii))) = mean_thetas(ii - burnIn), NaN over an empty range
};
__device__ __forceinline__ WavThetaStep wav_theta_step(double eta, double th_cur, double g, double delta, double dimX,
                                                       double min_eta, double max_eta, bool burn, double sum_eta,
                                                       double n_eta) {
#pragma clang fp contract(off)
    WavThetaStep t;
    const double etaii = eta + delta * (dimX / th_cur - g) * exp(eta);           // :180
    t.eta = fmin(fmax(etaii, min_eta), max_eta);                                 // :181
    t.th = exp(t.eta);                                                           // :182
    const double nan = __builtin_nan("");
    const double m0 = n_eta > 0.0 ? exp(sum_eta / n_eta) : nan;                  // exp(mean(eta(burnIn:ii-1))), empty: NaN
    t.sum_eta = burn ? sum_eta + t.eta : sum_eta;
    t.n_eta = burn ? n_eta + 1.0 : n_eta;
    t.mean = t.n_eta > 0.0 ? exp(t.sum_eta / t.n_eta) : nan;                     // :211
    t.tol = fabs(t.mean - m0) / m0;                                              // :199-200
    return t;
}

// ----------------------------- MYULA chain on the frame coefficients (wavelet_chain.hip) ---------
// What sbtv_SAPG_wavelet, sbtv_myula_wavelet and sbtv_SAPG_wavelet_semiblind share: the buffers of a chain, its start, the
// two halves of an operator pass and the step, enqueued on the context's stream.  Device pointers, but `noise`.
struct WavChain {
    WavPlan wp;
    BlurOp op;                   // operator layer "<prefix>": column spectrum of W X in op.S; op.Hs is filled by the caller
    int batch, nblk, nrb;        // element-wise workgroups per chain (wav_ew_blocks), row blocks per image (fft_rows_blocks)
    size_t P, cnt, dimX, ccnt;   // M N, P batch, (3J+1) P, dimX batch
    const double *yd, *x0d;      // y; the caller's start state or null (W'y)
    const double *noise;         // injected normals [step][batch][dimX] (host unless Z is null) or null: Philox
    double *X, *G, *img, *Z;     // state, gradient, image, staging of one step of host noise
};
// plan, staging of y / xw0 and the workspaces "<prefix>.y", .G, .X, .img, .Z, .S, .H, .Y
int wav_chain_buffers(sbtv_ctx *ctx, const char *prefix, const WavPlan &wp, int batch, const double *y, const double *xw0,
                      const double *noise, double *xw_last, int flags, WavChain *c);
// Ys = spectrum of y; X = xw0 or W'y (run_deblur_synthesis_L1.m:153)
int wav_chain_start(sbtv_ctx *ctx, const WavChain &c);
// S = column spectrum of W X; mom with k > 0: the image is sample k of the running moments (wav_synthesis)
int wav_chain_spectrum(sbtv_ctx *ctx, const WavChain &c, const MomArgs *mom = nullptr);
// the row pass on S with H, Y and (OP_GRAD only) D1, D2; ||B W X - y||^2 (and the OP_GRAD dot products) -> acc.  OP_RESID and
// OP_GRAD store nothing; OP_GRADF goes on to G = W' B'(B W X - y)
int wav_chain_rows(sbtv_ctx *ctx, const WavChain &c, int op, double *acc, const double2 *D1 = nullptr,
                   const double2 *D2 = nullptr);
// part [batch][nblk] = partial sums of ||X||_1
int wav_abs_sum(sbtv_ctx *ctx, const WavChain &c, double *part);
// where the step reads the two scalars of chain b: theta[b * stride], sigma2[b * stride] (device)
struct WavStepPar {
    const double *theta, *sigma2;
    int stride;
};
// One MYULA step of every chain (wav_step_kernel) with the normals of step rng.step: the injected ones, or Philox on (pair,
// rng.step, rng.chain0 + b).  part [batch][nblk] receives the partial sums of ||X_new||_1; mom with k > 0: X_new is sample k
// of the running moments of the coefficients.
int wav_chain_step(sbtv_ctx *ctx, const WavChain &c, const WavStepPar &par, double gam, double lamb, const RngArgs &rng,
                   double *part, const MomArgs *mom = nullptr);

// ---- SK-ROCK on the same target (wavelet_skrock.hip drives; the element-wise kernels live in wavelet_chain.hip)
// the drift of the Moreau-Yosida-smoothed posterior at one coefficient k with gradient g = (W'B'(B W K - y)) there:
//     D = (soft(k, T) - k)/lamb - g/s2,   T = lamb theta;   no contraction anywhere in it
__device__ __forceinline__ double wav_skrock_drift_nocontract(double k, double g, double T, double lamb, double s2) {
#pragma clang fp contract(off)
    return (wav_soft(k, T) - k) / lamb - g / s2;
}
// the scalars of one stage j of a step (include/sbtv.h, sbtv_skrock_wavelet); q = sqrt(2 delta)
struct WavSkrockStage {
    double mud;                  // mu_j delta
    double nu, kappa;            // nu_j, kappa_j; the first stage: unused, kappa_1 q
    double nu1q;                 // nu_1 q: the first stage forms P again with it, the last one forms P of the next step
};
// c.Z set: the staging buffer of host noise receives the normals of `step` (stream order)
int wav_skrock_noise(sbtv_ctx *ctx, const WavChain &c, unsigned step);
// P = X + (nu_1 q) Z with the normals of rng.step (injected, or Philox as in wav_chain_step): the first step of a call
int wav_skrock_perturb(sbtv_ctx *ctx, const WavChain &c, const double *X, double *P, double nu1q, const RngArgs &rng);
// One stage on every chain with G = c.G: U = K_{j-1}, V = K_{j-2}.
//   first: V = X, U = P (not read: P is formed again from X and the normals of rng.step); K_1 is written over U.
//   otherwise K_j is written over V.  last: K_j is the new sample: part [batch][nblk] receives the partial sums of
//   ||X_new||_1, mom with k > 0 accumulates it as sample k, and with next_p the normals of rng.step + 1 give
//   P_next = X_new + (nu_1 q) Z_next, written over U.
int wav_skrock_stage(sbtv_ctx *ctx, const WavChain &c, const WavStepPar &par, double lamb, double *U, double *V,
                     const WavSkrockStage &st, bool first, bool last, bool next_p, const RngArgs &rng, double *part,
                     const MomArgs *mom = nullptr);

#include "psf_taps.inc"   // psf_taps_point(): PSF formulas shared by host and device

}  // namespace sbtv

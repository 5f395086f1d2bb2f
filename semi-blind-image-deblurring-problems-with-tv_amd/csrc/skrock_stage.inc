// The element-wise kernels of one SK-ROCK step on the TV posterior (include/sbtv.h, sbtv_skrock): the perturbation, the stage
// kernels and the re-arming of the cold prox that follows each of them, and SkrockStepper, the host side of a step (below).
// Shared by skrock.hip (fixed parameters) and
// sapg_skrock.hip (the SAPG estimation with this step as its Markov kernel): both include this file inside their unnamed
// namespace, under `#pragma clang fp contract(off)`, as tv.hip includes tv_fused.inc; nothing here is relocatable device code.
constexpr int SKB = 256;          // lanes per workgroup of the element-wise kernels (grid: ew_blocks(P) x batch)

// the scalars of one stage j of a step (include/sbtv.h, sbtv_skrock_wavelet); q = sqrt(2 delta)
struct SkrockStage {
    double mud;                  // mu_j delta
    double nu, kappa;            // nu_j, kappa_j; the first stage: unused, kappa_1 q
    double nu1q;                 // nu_1 q: the first stage forms P again with it, the last one forms P of the next step
};

struct SkNoMom {};

// prox_reset(keep_cur = false) of chain b's control block, for the cold-start prox that follows the kernel
__device__ __forceinline__ void skrock_arm(const ProxArm &arm, int b) {
    ProxCtrl c = arm.ctrl[b];
    c.k = 0;
    c.done = 0;
    c.cur = 0;
    c.maxiter = arm.maxiter;
    c.redo = 0;
    c.f_valid = 0;
    c.err = 0.0;
    c.lambda = arm.lambda[b];
    c.tol = arm.tol;
    c.tau = arm.tau;
    arm.ctrl[b] = c;
}

// D(K) = (prox(K) - K)/lambda - g/sigma2 at one pixel, g = AT(A K - y)
__device__ __forceinline__ double skrock_drift_nocontract(double k, double p, double g, double lamb, double s2) {
    return (p - k) / lamb - g / s2;
}
// the perturbed state at one pixel: ONE expression for the perturb kernel, the first stage (which forms P again) and the
// last stage (P of the next step)
__device__ __forceinline__ double skrock_perturb_nocontract(double x, double z, double nu1q) { return x + nu1q * z; }

// P = X + (nu_1 q) Z for the first step of a call; every later P comes out of the last stage of the step before.  Z: injected
// normals in the layout of X, or null: pair q of chain b draws philox_normal_pair(q, step, chain0 + b, seed).
__global__ __launch_bounds__(SKB) void skrock_perturb_kernel(const double *__restrict__ X, double *__restrict__ Pout,
                                                             const double *__restrict__ Z, double nu1q, size_t P,
                                                             RngArgs rng, ProxArm arm) {
    const int b = blockIdx.y;
    if (arm.ctrl && blockIdx.x == 0 && threadIdx.x == 0) skrock_arm(arm, b);
    const size_t base = (size_t)b * P;
    for (size_t q = (size_t)blockIdx.x * SKB + threadIdx.x; q < P / 2; q += (size_t)gridDim.x * SKB) {
        const size_t o = base + 2 * q;
        const double2 xv = *reinterpret_cast<const double2 *>(X + o);
        const double2 zv = Z ? *reinterpret_cast<const double2 *>(Z + o)
                             : philox_normal_pair(q, rng.step, rng.chain0 + (unsigned)b, rng.seed);
        *reinterpret_cast<double2 *>(Pout + o) =
            make_double2(skrock_perturb_nocontract(xv.x, zv.x, nu1q), skrock_perturb_nocontract(xv.y, zv.y, nu1q));
    }
}

// the first stage at one pixel: K_1 = (x + (mu_1 delta) D(P)) + (kappa_1 q) z with P = x + (nu_1 q) z formed again
__device__ __forceinline__ double skrock_first_nocontract(double x, double p, double g, double z, double lamb, double s2,
                                                          const SkrockStage &st) {
    const double pp = skrock_perturb_nocontract(x, z, st.nu1q);
    return (x + st.mud * skrock_drift_nocontract(pp, p, g, lamb, s2)) + st.kappa * z;
}
// a later stage: K_j = ((mu_j delta) D(K_{j-1}) + nu_j K_{j-1}) + kappa_j K_{j-2}
__device__ __forceinline__ double skrock_stage_nocontract(double u, double v, double p, double g, double lamb, double s2,
                                                          const SkrockStage &st) {
    return (st.mud * skrock_drift_nocontract(u, p, g, lamb, s2) + st.nu * u) + st.kappa * v;
}

// One SK-ROCK stage of every chain, two pixels per lane as myula_plain_kernel; prox and grad are prox(K_{j-1}) and
// AT(A K_{j-1} - y) (FIRST: of P).
// FIRST: V = X is read, Z is drawn (or read) again with the counters of the perturbation, K_1 goes to U (P is not read).
// Otherwise U = K_{j-1} and V = K_{j-2} are read and K_j goes to V.  LAST: K_j is the new sample, with MOM sample mom.k of the
// running mean / M2; NEXT (every step but the last of a call): Z of step rng.step + 1 gives P of the next step, written over
// U, which this lane has just read.
// The compiler is asked for six waves per SIMD, as for wav_skrock_stage_kernel (myula_plain_kernel reaches five): left alone
// it may spread the divisions of the last stage next to the generator over more registers than that allows.
template <bool FIRST, bool LAST, bool NEXT, bool MOM>
__global__ __launch_bounds__(SKB) __attribute__((amdgpu_waves_per_eu(6))) void skrock_stage_kernel(
    double *__restrict__ U, double *__restrict__ V, const double *__restrict__ prox, const double *__restrict__ grad,
    const double *__restrict__ Z, const double *__restrict__ sigma2, double lamb, SkrockStage st, size_t P, RngArgs rng,
    ProxArm arm, std::conditional_t<MOM, MomArgs, SkNoMom> mom) {
    static_assert(!(FIRST && LAST) && (LAST || !(MOM || NEXT)), "a step has at least two stages; only the last one has a sample");
    const int b = blockIdx.y;
    if (arm.ctrl && blockIdx.x == 0 && threadIdx.x == 0) skrock_arm(arm, b);
    const size_t base = (size_t)b * P;
    const double s2 = sigma2[b];
    int k = 0;
    if constexpr (MOM) k = mom.k;
    const double rk = 1.0 / (double)(k > 0 ? k : 1);
    for (size_t q = (size_t)blockIdx.x * SKB + threadIdx.x; q < P / 2; q += (size_t)gridDim.x * SKB) {
        const size_t o = base + 2 * q;
        const double2 vv = *reinterpret_cast<const double2 *>(V + o);
        const double2 pv = *reinterpret_cast<const double2 *>(prox + o);
        const double2 gv = *reinterpret_cast<const double2 *>(grad + o);
        double2 r;
        if constexpr (FIRST) {
            const double2 zv = Z ? *reinterpret_cast<const double2 *>(Z + o)
                                 : philox_normal_pair(q, rng.step, rng.chain0 + (unsigned)b, rng.seed);
            r.x = skrock_first_nocontract(vv.x, pv.x, gv.x, zv.x, lamb, s2, st);
            r.y = skrock_first_nocontract(vv.y, pv.y, gv.y, zv.y, lamb, s2, st);
            *reinterpret_cast<double2 *>(U + o) = r;
        } else {
            const double2 uv = *reinterpret_cast<const double2 *>(U + o);
            r.x = skrock_stage_nocontract(uv.x, vv.x, pv.x, gv.x, lamb, s2, st);
            r.y = skrock_stage_nocontract(uv.y, vv.y, pv.y, gv.y, lamb, s2, st);
            *reinterpret_cast<double2 *>(V + o) = r;
        }
        if constexpr (LAST) {
            if constexpr (MOM) {
                if (k > 0) moments_pair(mom, o, r, k, rk);
            }
            if constexpr (NEXT) {
                const double2 zn = Z ? *reinterpret_cast<const double2 *>(Z + o)
                                     : philox_normal_pair(q, rng.step + 1u, rng.chain0 + (unsigned)b, rng.seed);
                *reinterpret_cast<double2 *>(U + o) = make_double2(skrock_perturb_nocontract(r.x, zn.x, st.nu1q),
                                                                   skrock_perturb_nocontract(r.y, zn.y, st.nu1q));
            }
        }
    }
}

// The host side of the steps of one call: the stage table, the two image buffers and the noise feed; it owns the perturb launch
// of the first step, the stage dispatch and the buffer parity.  Two image buffers alternate: stage j reads K_{j-1} (U) and
// K_{j-2} (V) and writes K_j over V; the last stage also writes the perturbed state P of the next step over U, so the new sample
// and P_next swap buffers when `stages` is odd.  The caller fills the fields up to `chain0`, calls table() and then step() once
// per sample; X is the buffer that holds the sample.  sigma2 and the lambda theta of `arm` are read on the device.
struct SkrockStepper {
    sbtv_ctx *ctx;
    const BlurOp *bop;
    const ProxPlan *pp;
    ProxArm arm;
    NoiseFeed nz;
    double *X, *Pb;              // the sample; the perturbed state of the next step
    double *prox, *grad, *acc_g; // prox and gradient of a stage's input; the residual sums of the gradient passes (not used)
    const double *sig_d;         // [batch] (device)
    double *pm_mean, *pm_m2;     // running mean / M2 of the samples [batch][P], or null
    double lambda;
    size_t P;
    int batch, stages, chambolleit;
    unsigned long long seed;
    unsigned chain0;
    unsigned done = 0;           // steps taken: the counter of the next one (steps count from 0)
    std::vector<SkrockStage> st;

    // the coefficient table and the scalars of the stages for the step dt
    int table(double eta, double dt) {
        std::vector<double> mu(stages), nu(stages), kappa(stages);
        SBTV_TRY(sbtv_skrock_coefficients(stages, eta, mu.data(), nu.data(), kappa.data(), nullptr, nullptr));
        const double q = sqrt(2 * dt), nu1q = nu[0] * q;
        st.assign(stages, SkrockStage{});
        st[0] = SkrockStage{mu[0] * dt, 0.0, kappa[0] * q, nu1q};
        for (int j = 1; j < stages; ++j) st[j] = SkrockStage{mu[j] * dt, nu[j], kappa[j], nu1q};
        return 0;
    }
    // one stage: the drift at U (prox and gradient with the current H), then the stage kernel
    int stage(double *U, double *V, int j, bool next_p, const RngArgs &r, const MomArgs *mc) {
        const bool first = j == 1, last = j == stages, np = last && next_p, mo_on = last && mc && mc->k > 0;
        SBTV_TRY(prox_iterate(ctx, *pp, U, chambolleit, prox, true));
        SBTV_TRY(op_gradf(ctx, *bop, U, acc_g, grad));
        const double *zd = first ? nz.ptr(r.step) : (np ? nz.ptr(r.step + 1u) : nullptr);
        const SkrockStage &sj = st[j - 1];
        const dim3 grid(ew_blocks(P), batch), block(SKB);
#define SBTV_SKROCK_STAGE(F, L, NX, MO, momarg)                                                                           \
    hipLaunchKernelGGL((skrock_stage_kernel<F, L, NX, MO>), grid, block, 0, ctx->stream, U, V, (const double *)prox,         \
                       (const double *)grad, zd, sig_d, lambda, sj, P, r, arm, momarg)
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
    }
    // X <- SKROCK_step(X); momk > 0: the new sample is sample momk of the moments; more: another step follows, so the last
    // stage forms its perturbed state
    int step(int momk, bool more) {
        const RngArgs r{seed, done, chain0, nullptr};
        if (done == 0) {
            SBTV_TRY(nz.stage(0));
            hipLaunchKernelGGL(skrock_perturb_kernel, dim3(ew_blocks(P), batch), dim3(SKB), 0, ctx->stream, (const double *)X, Pb,
                               nz.ptr(0), st[0].nu1q, P, r, arm);
            SBTV_HIP(ctx, hipGetLastError());
        }
        double *U = Pb, *V = X;                                              // K_{j-1} (stage 1: P), K_{j-2}
        SBTV_TRY(stage(U, V, 1, false, r, nullptr));
        if (more) SBTV_TRY(nz.stage(done + 1u));                             // after FIRST, before LAST
        for (int j = 2; j <= stages; ++j) {
            const MomArgs mc{pm_mean, pm_m2, j == stages ? momk : 0, nullptr, 1, 1};
            SBTV_TRY(stage(U, V, j, more, r, &mc));
            std::swap(U, V);                                                 // U = K_j, V = K_{j-1} (after the last: P_next)
        }
        X = U;
        Pb = V;
        ++done;
        return 0;
    }
};

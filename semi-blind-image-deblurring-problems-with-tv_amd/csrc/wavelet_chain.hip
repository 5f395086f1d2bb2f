// The MYULA chain on the coefficients of the redundant wavelet frame, as far as its three drivers share it (DESIGN.md
// §3.9-3.11): sbtv_SAPG_wavelet (wavelet_sapg.hip), sbtv_myula_wavelet (wavelet_myula.hip) and sbtv_SAPG_wavelet_semiblind
// (wavelet_sapg_sb.hip).  The buffers of a chain, the spectrum of y and the start state, the two halves of an operator pass
// (synthesis + forward column pass; row pass, and for the gradient the inverse column pass + analysis), and the two
// element-wise kernels: the library is built without relocatable device code, so a kernel is launched from the unit that
// defines it and the drivers reach these through the host functions of sbtv_internal.h.  The drivers keep what differs:
// the order of the passes, where theta and sigma2 live, the update / trace kernels.
// The SK-ROCK chain on the same target (sbtv_skrock_wavelet in wavelet_skrock.hip) runs the same passes on
// either of its two coefficient buffers; its perturbation and stage kernels stand here next to wav_step_kernel.
#include <cmath>
#include <string>
#include <type_traits>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

// ||X||_1 of the start state: partials [batch][gridDim.x]
__global__ __launch_bounds__(WAV_EWB) void wav_abs_sum_kernel(const double *__restrict__ X, size_t dimX,
                                                               double *__restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const double *x = X + (size_t)b * dimX;
    double a = 0.0;
    for (size_t q = (size_t)blockIdx.x * WAV_EWB + threadIdx.x; q < dimX / 2; q += (size_t)gridDim.x * WAV_EWB) {
        const double2 v = *reinterpret_cast<const double2 *>(x + 2 * q);
        a += fabs(v.x) + fabs(v.y);
    }
    a = wav_block_sum(a, red);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = a;
}

struct WavNoMom {};

// One MYULA step of every chain (SAPG_algorithm_1.m:133,174) on the coefficients, two per lane (dimX is even: an odd pixel
// count is refused), at the chain's own theta_b / sigma2_b (par):
//     X = X + gamma (soft(X, lambda theta_b) - X) / lambda - gamma G / sigma2_b + sqrt(2 gamma) Z
// The prox is never stored: a driver whose theta moves passes the theta the reference formed it with, which lags one
// iteration.  G = W' B'(B W X - y).  Z: injected normals in the layout of X, or null: pair q of chain b draws
// philox_normal_pair(q, step, chain0 + b, seed).  X and G are read once, X is written once; part [batch][gridDim.x]
// receives the workgroup's sum of |X_new|.  MOM: X_new is also sample mom.k of the running mean / M2 of the coefficients;
// the plain instantiation carries no MomArgs.
template <bool MOM>
__global__ __launch_bounds__(WAV_EWB) void wav_step_kernel(double *__restrict__ X, const double *__restrict__ G,
                                                            const double *__restrict__ Z, WavStepPar par, double gam,
                                                            double lamb, double sq2g, size_t dimX, RngArgs rng,
                                                            double *__restrict__ part,
                                                            std::conditional_t<MOM, MomArgs, WavNoMom> mom) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * dimX, pb = (size_t)b * par.stride;
    const double T = lamb * par.theta[pb], s2 = par.sigma2[pb];
    int k = 0;
    if constexpr (MOM) k = mom.k;
    const double rk = 1.0 / (double)(k > 0 ? k : 1);
    double a = 0.0;
    for (size_t q = (size_t)blockIdx.x * WAV_EWB + threadIdx.x; q < dimX / 2; q += (size_t)gridDim.x * WAV_EWB) {
        const size_t o = base + 2 * q;
        const double2 xv = *reinterpret_cast<const double2 *>(X + o);
        const double2 gv = *reinterpret_cast<const double2 *>(G + o);
        const double2 zv = Z ? *reinterpret_cast<const double2 *>(Z + o)
                             : philox_normal_pair(q, rng.step, rng.chain0 + (unsigned)b, rng.seed);
        double2 r;
        r.x = wav_myula_nocontract(xv.x, gv.x, zv.x, T, gam, lamb, s2, sq2g);
        r.y = wav_myula_nocontract(xv.y, gv.y, zv.y, T, gam, lamb, s2, sq2g);
        *reinterpret_cast<double2 *>(X + o) = r;
        if constexpr (MOM) {
            if (k > 0) moments_pair(mom, o, r, k, rk);
        }
        a += fabs(r.x) + fabs(r.y);
    }
    a = wav_block_sum(a, red);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = a;
}

// SK-ROCK (include/sbtv.h, sbtv_skrock_wavelet): P = X + (nu_1 q) Z for the first step of a call; every later P comes out of
// the last stage of the step before.  Z as in wav_step_kernel.
__global__ __launch_bounds__(WAV_EWB) void wav_skrock_perturb_kernel(const double *__restrict__ X, double *__restrict__ P,
                                                                      const double *__restrict__ Z, double nu1q, size_t dimX,
                                                                      RngArgs rng) {
    const int b = blockIdx.y;
    const size_t base = (size_t)b * dimX;
    for (size_t q = (size_t)blockIdx.x * WAV_EWB + threadIdx.x; q < dimX / 2; q += (size_t)gridDim.x * WAV_EWB) {
        const size_t o = base + 2 * q;
        const double2 xv = *reinterpret_cast<const double2 *>(X + o);
        const double2 zv = Z ? *reinterpret_cast<const double2 *>(Z + o)
                             : philox_normal_pair(q, rng.step, rng.chain0 + (unsigned)b, rng.seed);
        *reinterpret_cast<double2 *>(P + o) = make_double2(xv.x + nu1q * zv.x, xv.y + nu1q * zv.y);
    }
}

// the first stage at one coefficient: K_1 = (x + (mu_1 delta) D(P)) + (kappa_1 q) z with P = x + (nu_1 q) z formed again
__device__ __forceinline__ double wav_skrock_first_nocontract(double x, double g, double z, double T, double lamb, double s2,
                                                              const WavSkrockStage &st) {
    const double p = x + st.nu1q * z;
    return (x + st.mud * wav_skrock_drift_nocontract(p, g, T, lamb, s2)) + st.kappa * z;
}
// a later stage: K_j = ((mu_j delta) D(K_{j-1}) + nu_j K_{j-1}) + kappa_j K_{j-2}
__device__ __forceinline__ double wav_skrock_stage_nocontract(double u, double v, double g, double T, double lamb, double s2,
                                                              const WavSkrockStage &st) {
    return (st.mud * wav_skrock_drift_nocontract(u, g, T, lamb, s2) + st.nu * u) + st.kappa * v;
}

// One SK-ROCK stage of every chain, two coefficients per lane as wav_step_kernel; G is the gradient at K_{j-1} (FIRST: at P).
// FIRST: V = X is read, Z is drawn (or read) again with the counters of the perturbation, K_1 goes to U (P is not read).
// Otherwise U = K_{j-1} and V = K_{j-2} are read and K_j goes to V.  LAST: K_j is the new sample: part and, with MOM, the
// moments as in wav_step_kernel; NEXT (every step but the last of a call): Z of step rng.step + 1 gives P of the next step,
// written over U, which this lane has just read.
// The compiler is asked for the six waves per SIMD of wav_step_kernel: left alone it spreads the four divisions of the last stage
// over 100+ registers next to the generator (four waves); with the bound it needs 78 and no scratch.
template <bool FIRST, bool LAST, bool NEXT, bool MOM>
__global__ __launch_bounds__(WAV_EWB) __attribute__((amdgpu_waves_per_eu(6))) void wav_skrock_stage_kernel(
    double *__restrict__ U, double *__restrict__ V, const double *__restrict__ G, const double *__restrict__ Z, WavStepPar par,
    double lamb, WavSkrockStage st, size_t dimX, RngArgs rng, double *__restrict__ part,
    std::conditional_t<MOM, MomArgs, WavNoMom> mom) {
    static_assert(!(FIRST && LAST) && (LAST || !(MOM || NEXT)), "a step has at least two stages; only the last one has a sample");
    __shared__ double red[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * dimX, pb = (size_t)b * par.stride;
    const double T = lamb * par.theta[pb], s2 = par.sigma2[pb];
    int k = 0;
    if constexpr (MOM) k = mom.k;
    const double rk = 1.0 / (double)(k > 0 ? k : 1);
    double a = 0.0;
    for (size_t q = (size_t)blockIdx.x * WAV_EWB + threadIdx.x; q < dimX / 2; q += (size_t)gridDim.x * WAV_EWB) {
        const size_t o = base + 2 * q;
        const double2 vv = *reinterpret_cast<const double2 *>(V + o);
        const double2 gv = *reinterpret_cast<const double2 *>(G + o);
        double2 r;
        if constexpr (FIRST) {
            const double2 zv = Z ? *reinterpret_cast<const double2 *>(Z + o)
                                 : philox_normal_pair(q, rng.step, rng.chain0 + (unsigned)b, rng.seed);
            r.x = wav_skrock_first_nocontract(vv.x, gv.x, zv.x, T, lamb, s2, st);
            r.y = wav_skrock_first_nocontract(vv.y, gv.y, zv.y, T, lamb, s2, st);
            *reinterpret_cast<double2 *>(U + o) = r;
        } else {
            const double2 uv = *reinterpret_cast<const double2 *>(U + o);
            r.x = wav_skrock_stage_nocontract(uv.x, vv.x, gv.x, T, lamb, s2, st);
            r.y = wav_skrock_stage_nocontract(uv.y, vv.y, gv.y, T, lamb, s2, st);
            *reinterpret_cast<double2 *>(V + o) = r;
        }
        if constexpr (LAST) {
            if constexpr (MOM) {
                if (k > 0) moments_pair(mom, o, r, k, rk);
            }
            a += fabs(r.x) + fabs(r.y);
            if constexpr (NEXT) {
                const double2 zn = Z ? *reinterpret_cast<const double2 *>(Z + o)
                                     : philox_normal_pair(q, rng.step + 1u, rng.chain0 + (unsigned)b, rng.seed);
                *reinterpret_cast<double2 *>(U + o) = make_double2(r.x + st.nu1q * zn.x, r.y + st.nu1q * zn.y);
            }
        }
    }
    if constexpr (LAST) {
        a = wav_block_sum(a, red);
        if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = a;
    }
}

}  // namespace

int wav_chain_buffers(sbtv_ctx *ctx, const char *prefix, const WavPlan &wp, int batch, const double *y, const double *xw0,
                      const double *noise, double *xw_last, int flags, WavChain *c) {
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    SBTV_TRY(op_open(ctx, prefix, wp.M, wp.N, batch, "Y", &c->op));
    c->wp = wp;
    c->batch = batch;
    c->P = (size_t)wp.M * wp.N;
    c->cnt = c->P * batch;
    c->dimX = c->P * wp.bands();
    c->ccnt = c->dimX * batch;
    c->nblk = wav_ew_blocks(c->dimX);
    c->nrb = fft_rows_blocks(c->op.fp);
    c->noise = noise;
    c->Z = nullptr;
    const std::string p(prefix);
    SBTV_TRY(stage_in(ctx, (p + ".y").c_str(), y, c->cnt, flags, &c->yd));
    SBTV_TRY(stage_in(ctx, (p + ".G").c_str(), xw0, c->ccnt, flags, &c->x0d));     // staged where the gradient goes later
    SBTV_TRY(stage_out_buf(ctx, (p + ".X").c_str(), xw_last, c->ccnt, flags, &c->X));
    SBTV_TRY(ws_get_t(ctx, (p + ".G").c_str(), c->ccnt, &c->G));
    SBTV_TRY(ws_get_t(ctx, (p + ".img").c_str(), c->cnt, &c->img));
    if (noise && !(flags & SBTV_DEVICE_PTRS)) SBTV_TRY(ws_get_t(ctx, (p + ".Z").c_str(), c->ccnt, &c->Z));
    return 0;
}

int wav_chain_start(sbtv_ctx *ctx, const WavChain &c) {
    SBTV_TRY(op_spectrum(ctx, c.op.fp, c.yd, nullptr, c.op.S, c.op.Ys));
    if (!c.x0d) return wav_analysis(ctx, c.wp, c.yd, c.X, c.batch);
    if (c.x0d != c.X) SBTV_HIP(ctx, hipMemcpyAsync(c.X, c.x0d, sizeof(double) * c.ccnt, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int wav_chain_spectrum(sbtv_ctx *ctx, const WavChain &c, const MomArgs *mom) {
    SBTV_TRY(wav_synthesis(ctx, c.wp, c.X, c.img, c.batch, mom && mom->k > 0 ? mom : nullptr));
    return fft_cols_fwd(ctx, c.op.fp, c.img, nullptr, c.op.S);
}

int wav_chain_rows(sbtv_ctx *ctx, const WavChain &c, int op, double *acc, const double2 *D1, const double2 *D2) {
    RowsArgs ra{};
    ra.dir_fwd = 1;
    ra.dir_inv = op == OP_GRADF;
    ra.op = op;
    ra.H = c.op.Hs;
    ra.Y = c.op.Ys;
    ra.D1 = op == OP_GRAD ? D1 : nullptr;
    ra.D2 = op == OP_GRAD ? D2 : nullptr;
    ra.acc = acc;
    SBTV_TRY(fft_rows(ctx, c.op.fp, c.op.S, ra.dir_inv ? c.op.S : nullptr, ra));
    if (!ra.dir_inv) return 0;
    SBTV_TRY(fft_cols_inv(ctx, c.op.fp, c.op.S, c.img, c.op.inv_scale));
    return wav_analysis(ctx, c.wp, c.img, c.G, c.batch);
}

int wav_abs_sum(sbtv_ctx *ctx, const WavChain &c, double *part) {
    hipLaunchKernelGGL(wav_abs_sum_kernel, dim3(c.nblk, c.batch), dim3(WAV_EWB), 0, ctx->stream, (const double *)c.X, c.dimX,
                       part);
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

int wav_chain_step(sbtv_ctx *ctx, const WavChain &c, const WavStepPar &par, double gam, double lamb, const RngArgs &rng,
                   double *part, const MomArgs *mom) {
    const double *zd = c.noise ? c.noise + (size_t)rng.step * c.ccnt : nullptr;
    if (c.Z) {
        SBTV_HIP(ctx, hipMemcpyAsync(c.Z, zd, sizeof(double) * c.ccnt, hipMemcpyHostToDevice, ctx->stream));
        zd = c.Z;
    }
    const dim3 grid(c.nblk, c.batch), block(WAV_EWB);
    const double sq2g = sqrt(2 * gam);
    if (mom && mom->k > 0)
        hipLaunchKernelGGL(wav_step_kernel<true>, grid, block, 0, ctx->stream, c.X, (const double *)c.G, zd, par, gam, lamb,
                           sq2g, c.dimX, rng, part, *mom);
    else
        hipLaunchKernelGGL(wav_step_kernel<false>, grid, block, 0, ctx->stream, c.X, (const double *)c.G, zd, par, gam, lamb,
                           sq2g, c.dimX, rng, part, WavNoMom{});
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

int wav_skrock_noise(sbtv_ctx *ctx, const WavChain &c, unsigned step) {
    if (!c.Z) return 0;
    SBTV_HIP(ctx, hipMemcpyAsync(c.Z, c.noise + (size_t)step * c.ccnt, sizeof(double) * c.ccnt, hipMemcpyHostToDevice,
                                 ctx->stream));
    return 0;
}

// the normals of `step` as the kernels read them: the staging buffer (wav_skrock_noise filled it), the caller's device array,
// or null: Philox
static const double *wav_skrock_z(const WavChain &c, unsigned step) {
    if (c.Z) return c.Z;
    return c.noise ? c.noise + (size_t)step * c.ccnt : nullptr;
}

int wav_skrock_perturb(sbtv_ctx *ctx, const WavChain &c, const double *X, double *P, double nu1q, const RngArgs &rng) {
    hipLaunchKernelGGL(wav_skrock_perturb_kernel, dim3(c.nblk, c.batch), dim3(WAV_EWB), 0, ctx->stream, X, P,
                       wav_skrock_z(c, rng.step), nu1q, c.dimX, rng);
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

int wav_skrock_stage(sbtv_ctx *ctx, const WavChain &c, const WavStepPar &par, double lamb, double *U, double *V,
                     const WavSkrockStage &st, bool first, bool last, bool next_p, const RngArgs &rng, double *part,
                     const MomArgs *mom) {
    if (first && last) return fail(ctx, SBTV_ERR_BADARG, "wav_skrock_stage: a step has at least two stages");
    const dim3 grid(c.nblk, c.batch), block(WAV_EWB);
    const double *G = c.G;
    const bool np = last && next_p;
    const double *zd = first ? wav_skrock_z(c, rng.step) : (np ? wav_skrock_z(c, rng.step + 1u) : nullptr);
#define SBTV_SKROCK_STAGE(F, L, NX, MO, momarg)                                                                        \
    hipLaunchKernelGGL((wav_skrock_stage_kernel<F, L, NX, MO>), grid, block, 0, ctx->stream, U, V, G, zd, par, lamb, st,   \
                       c.dimX, rng, part, momarg)
    const bool mo = mom && mom->k > 0;
    if (first)
        SBTV_SKROCK_STAGE(true, false, false, false, WavNoMom{});
    else if (!last)
        SBTV_SKROCK_STAGE(false, false, false, false, WavNoMom{});
    else if (np && mo)
        SBTV_SKROCK_STAGE(false, true, true, true, *mom);
    else if (np)
        SBTV_SKROCK_STAGE(false, true, true, false, WavNoMom{});
    else if (mo)
        SBTV_SKROCK_STAGE(false, true, false, true, *mom);
    else
        SBTV_SKROCK_STAGE(false, true, false, false, WavNoMom{});
#undef SBTV_SKROCK_STAGE
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace sbtv

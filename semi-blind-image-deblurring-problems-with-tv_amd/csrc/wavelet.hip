// The redundant (undecimated, translation-invariant) 2-D wavelet frame of the wavelet-l1 solver:
//   analysis   W' : image -> 3J+1 bands   (mrdwt_TI2D,  SALSA/mrdwt_TI2D.m with its rescaling applied)
//   synthesis  W  : 3J+1 bands -> image   (mirdwt_TI2D, SALSA/mirdwt_TI2D.m), the exact adjoint: W W' = I
// plus the element-wise soft threshold (SALSA/soft.m).  The Rice Wavelet Toolbox MEX behind the reference's wrappers is not
// shipped (SALSA/mrdwt.m is a comment block), so the transform is stated here: for level j = 1..J, stride s = 2^(j-1),
//   lo[i] = (1/sqrt 2) sum_k h0[k] a[(i + s k) mod n],   hi[i] = (1/sqrt 2) sum_k h1[k] a[(i + s k) mod n],
//   h0 = h, h1[k] = (-1)^k h[K-1-k], along dimension 1 (the contiguous index) and then along dimension 2.
//
// One launch per level.  A workgroup filters one 2-D tile held in LDS in both directions: analysis reads a_{j-1} once and
// writes a_j and the three detail bands once, synthesis reads the four bands once and writes a_{j-1} once; the lo / hi
// intermediates live in LDS only.
//
// Tile geometry.  Level j only couples samples whose indices differ by multiples of s, so a tile need not be contiguous:
// along one dimension it is the indices  base + a s + q,  q < Q (a run of Q neighbours), a < A + K - 1
// (A output steps and K - 1 halo steps), Q a power of two that divides s.  Its LDS index is a Q + q, so tap k sits k Q further
// on.  With Q = s the tile is the contiguous range of s A indices with its halo of (K - 1) s; Q is capped (CAP1 / CAP2
// below) so that the halo, (K - 1) Q, and with it the LDS footprint stay bounded however deep the decomposition goes: beyond
// the cap the tile is a comb of Q-runs.  Every output index i = s alpha + rho belongs to exactly one tile, (alpha / A, rho /
// Q); indices wrap modulo the image size on load and tiles are cut at the image size on store, so any M, N works.
#include <cmath>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

constexpr int WT1 = 64;        // outputs of a tile along dimension 1: one per lane
constexpr int WNW = 4;         // waves per workgroup
constexpr int WA_T2 = 32;      // outputs of an analysis tile along dimension 2
constexpr int WS_T2 = 16;      // ... of a synthesis tile (it holds two band tiles and lo / hi with the dimension-1 halo)

// largest run Q along dimension 1 / 2 for filter length K (LDS of either kernel <= 80 KB: two workgroups per CU)
__host__ __device__ constexpr int wav_cap1(int K) { return K == 2 ? 16 : K == 4 ? 8 : 4; }
__host__ __device__ constexpr int wav_cap2(int K) { return K <= 4 ? 4 : 2; }

struct WavTaps {
    double f0[8], f1[8];       // h0 / sqrt 2, h1 / sqrt 2
};

struct WavGeom {
    int M, N;
    int ls;                    // log2 of the stride s
    int lq1, lq2;              // log2 of the runs Q1, Q2
    int nr1, nr2;              // runs per stride: s / Q1, s / Q2 (tiles along a dimension = blocks of A steps x nr)
    size_t img_in, img_out;    // doubles between the images of a batch on the image side / on the band side
};

__device__ __forceinline__ int wav_wrap(int i, int n) {
    if (i < 0) i += n;
    if (i >= n) i %= n;
    return i;
}

// global index of LDS index l (= a Q + q) of a tile that starts at `base`; `back`: halo steps in front of the tile
__device__ __forceinline__ int wav_index(int l, int base, int lq, int ls, int back) {
    return base + ((l >> lq) - back) * (1 << ls) + (l & ((1 << lq) - 1));
}

// a tile's first index: tile t = (block of A steps) * nr + (run of the stride)
__device__ __forceinline__ int wav_base(int t, int nr, int T, int lq, int ls) {
    const int blk = t / nr, run = t - blk * nr;
    return ((blk * (T >> lq)) << ls) + (run << lq);
}

// ---- analysis: a_{j-1} -> a_j (ll), lh, hl, hh -----------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(WNW * 64) void wav_analysis_kernel(const double *__restrict__ in, double *__restrict__ ll,
                                                                 double *__restrict__ lh, double *__restrict__ hl,
                                                                 double *__restrict__ hh, size_t ll_img, WavTaps tp,
                                                                 WavGeom g) {
    constexpr int L1 = WT1 + wav_cap1(K) * (K - 1), L2 = WA_T2 + wav_cap2(K) * (K - 1);
    __shared__ double tile[L2 * L1];
    __shared__ double lo[L2 * WT1], hi[L2 * WT1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q1 = 1 << g.lq1, q2 = 1 << g.lq2;
    const int n1 = WT1 + q1 * (K - 1), n2 = WA_T2 + q2 * (K - 1);      // the tile with its halo
    const int b1 = wav_base(blockIdx.x, g.nr1, WT1, g.lq1, g.ls), b2 = wav_base(blockIdx.y, g.nr2, WA_T2, g.lq2, g.ls);
    in += (size_t)blockIdx.z * g.img_in;
    const size_t ob = (size_t)blockIdx.z * g.img_out;
    for (int c = w; c < n2; c += WNW) {
        const int gc = wav_wrap(wav_index(c, b2, g.lq2, g.ls, 0), g.N);
        for (int r = lane; r < n1; r += 64) {
            const int gr = wav_wrap(wav_index(r, b1, g.lq1, g.ls, 0), g.M);
            tile[c * L1 + r] = in[(size_t)gc * g.M + gr];
        }
    }
    __syncthreads();
    for (int c = w; c < n2; c += WNW) {                                // dimension 1
        double a = 0.0, d = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double v = tile[c * L1 + lane + k * q1];
            a += tp.f0[k] * v;
            d += tp.f1[k] * v;
        }
        lo[c * WT1 + lane] = a;
        hi[c * WT1 + lane] = d;
    }
    __syncthreads();
    const int gr = wav_index(lane, b1, g.lq1, g.ls, 0);
    for (int c = w; c < WA_T2; c += WNW) {                             // dimension 2
        const int gc = wav_index(c, b2, g.lq2, g.ls, 0);
        double v_ll = 0.0, v_lh = 0.0, v_hl = 0.0, v_hh = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double a = lo[(c + k * q2) * WT1 + lane], d = hi[(c + k * q2) * WT1 + lane];
            v_ll += tp.f0[k] * a;
            v_lh += tp.f1[k] * a;
            v_hl += tp.f0[k] * d;
            v_hh += tp.f1[k] * d;
        }
        if (gr < g.M && gc < g.N) {
            const size_t o = (size_t)gc * g.M + gr;
            ll[(size_t)blockIdx.z * ll_img + o] = v_ll;
            lh[ob + o] = v_lh;
            hl[ob + o] = v_hl;
            hh[ob + o] = v_hh;
        }
    }
}

// ---- synthesis: a_j (ll), lh, hl, hh -> a_{j-1} (transposed filters: index i - s k) -------------------------------
// ONE body for the plain kernel and for the one that also accumulates the posterior moments of the image it stores (MOM,
// level 1 only: sample k of mom.mean / mom.m2 [batch][M N]), so both store the same bits
template <int K, bool MOM>
__device__ __forceinline__ void wav_synthesis_body(const double *__restrict__ ll, const double *__restrict__ lh,
                                                   const double *__restrict__ hl, const double *__restrict__ hh,
                                                   size_t ll_img, double *__restrict__ out, const WavTaps &tp,
                                                   const WavGeom &g, const MomArgs &mom) {
    constexpr int L1 = WT1 + wav_cap1(K) * (K - 1), L2 = WS_T2 + wav_cap2(K) * (K - 1);
    __shared__ double ta[L2 * L1], tb[L2 * L1];
    __shared__ double lo[WS_T2 * L1], hi[WS_T2 * L1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q1 = 1 << g.lq1, q2 = 1 << g.lq2;
    const int n1 = WT1 + q1 * (K - 1), n2 = WS_T2 + q2 * (K - 1);
    const int b1 = wav_base(blockIdx.x, g.nr1, WT1, g.lq1, g.ls), b2 = wav_base(blockIdx.y, g.nr2, WS_T2, g.lq2, g.ls);
    const size_t ib = (size_t)blockIdx.z * g.img_in;
    ll += (size_t)blockIdx.z * ll_img;
    for (int half = 0; half < 2; ++half) {
        const double *pa = half ? hl + ib : ll, *pb = half ? hh + ib : lh + ib;
        double *dst = half ? hi : lo;
        if (half) __syncthreads();                                     // the first pair has been consumed
        for (int c = w; c < n2; c += WNW) {
            const int gc = wav_wrap(wav_index(c, b2, g.lq2, g.ls, K - 1), g.N);
            for (int r = lane; r < n1; r += 64) {
                const int gr = wav_wrap(wav_index(r, b1, g.lq1, g.ls, K - 1), g.M);
                const size_t o = (size_t)gc * g.M + gr;
                ta[c * L1 + r] = pa[o];
                tb[c * L1 + r] = pb[o];
            }
        }
        __syncthreads();
        for (int c = w; c < WS_T2; c += WNW) {                         // dimension 2, every row of the tile and its halo
            for (int r = lane; r < n1; r += 64) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int cc = c + (K - 1 - k) * q2;
                    v += tp.f0[k] * ta[cc * L1 + r] + tp.f1[k] * tb[cc * L1 + r];
                }
                dst[c * L1 + r] = v;
            }
        }
    }
    __syncthreads();
    const int gr = wav_index(lane, b1, g.lq1, g.ls, 0);
    const double rk = 1.0 / (double)(MOM && mom.k > 0 ? mom.k : 1);
    for (int c = w; c < WS_T2; c += WNW) {                             // dimension 1
        const int gc = wav_index(c, b2, g.lq2, g.ls, 0);
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int rr = lane + (K - 1 - k) * q1;
            v += tp.f0[k] * lo[c * L1 + rr] + tp.f1[k] * hi[c * L1 + rr];
        }
        if (gr < g.M && gc < g.N) {
            out[(size_t)blockIdx.z * g.img_out + (size_t)gc * g.M + gr] = v;
            if (MOM) {
                const size_t o = ((size_t)blockIdx.z * g.N + gc) * g.M + gr;
                double mu = 0.0, s = 0.0;
                if (mom.k > 1) {
                    mu = mom.mean[o];
                    s = mom.m2[o];
                }
                welford_nocontract(mu, s, v, mom.k, rk);
                mom.mean[o] = mu;
                mom.m2[o] = s;
            }
        }
    }
}

template <int K>
__global__ __launch_bounds__(WNW * 64) void wav_synthesis_kernel(const double *__restrict__ ll, const double *__restrict__ lh,
                                                                  const double *__restrict__ hl, const double *__restrict__ hh,
                                                                  size_t ll_img, double *__restrict__ out, WavTaps tp,
                                                                  WavGeom g) {
    wav_synthesis_body<K, false>(ll, lh, hl, hh, ll_img, out, tp, g, MomArgs{});
}

// level-1 synthesis with a Welford epilogue: the pixel about to be stored is sample mom.k >= 1 of the running mean / M2
// (k = 1 starts them without reading): 32 B per pixel on top of the plain kernel, no extra launch, no re-read of the image
template <int K>
__global__ __launch_bounds__(WNW * 64) void wav_synthesis_moments_kernel(const double *__restrict__ ll,
                                                                          const double *__restrict__ lh,
                                                                          const double *__restrict__ hl,
                                                                          const double *__restrict__ hh, size_t ll_img,
                                                                          double *__restrict__ out, WavTaps tp, WavGeom g,
                                                                          MomArgs mom) {
    wav_synthesis_body<K, true>(ll, lh, hl, hh, ll_img, out, tp, g, mom);
}

// ---- soft threshold, one T per image ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wav_soft_kernel(const double *__restrict__ x, const double *__restrict__ T,
                                                        double *__restrict__ out, size_t P) {
    const double t = T[blockIdx.y];
    x += (size_t)blockIdx.y * P;
    out += (size_t)blockIdx.y * P;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (size_t)gridDim.x * 256)
        out[i] = wav_soft(x[i], t);
}

WavGeom wav_geom(const WavPlan &pl, int level) {
    WavGeom g;
    g.M = pl.M;
    g.N = pl.N;
    g.ls = level - 1;
    const int s = 1 << g.ls;
    const int q1 = s < wav_cap1(pl.K) ? s : wav_cap1(pl.K), q2 = s < wav_cap2(pl.K) ? s : wav_cap2(pl.K);
    g.lq1 = ilog2(q1);
    g.lq2 = ilog2(q2);
    g.nr1 = s / q1;
    g.nr2 = s / q2;
    g.img_in = g.img_out = 0;
    return g;
}

// tiles along a dimension of n samples: blocks of T / Q steps over the ceil(n / s) steps of a run, times the runs of a stride
inline unsigned wav_tiles(int n, int ls, int lq, int nr, int T) {
    const int steps = (n + (1 << ls) - 1) >> ls, A = T >> lq;
    return (unsigned)(((steps + A - 1) / A) * nr);
}

// the grids of the two launches of a level (sbtv_diag_wavelet_geometry reports them from here)
inline dim3 wav_grid_analysis(const WavPlan &pl, const WavGeom &g, int batch) {
    return dim3(wav_tiles(pl.M, g.ls, g.lq1, g.nr1, WT1), wav_tiles(pl.N, g.ls, g.lq2, g.nr2, WA_T2), (unsigned)batch);
}

inline dim3 wav_grid_synthesis(const WavPlan &pl, const WavGeom &g, int batch) {
    return dim3(wav_tiles(pl.M, g.ls, g.lq1, g.nr1, WT1), wav_tiles(pl.N, g.ls, g.lq2, g.nr2, WS_T2), (unsigned)batch);
}

template <int K>
int wav_level_analysis(sbtv_ctx *ctx, const WavPlan &pl, int level, const double *in, size_t in_img, double *ll,
                       size_t ll_img, double *det, int batch) {
    WavGeom g = wav_geom(pl, level);
    const size_t P = (size_t)pl.M * pl.N;
    g.img_in = in_img;
    g.img_out = (size_t)pl.bands() * P;
    WavTaps tp;
    for (int k = 0; k < 8; ++k) {
        tp.f0[k] = pl.f0[k];
        tp.f1[k] = pl.f1[k];
    }
    const dim3 grid = wav_grid_analysis(pl, g, batch);
    hipLaunchKernelGGL(wav_analysis_kernel<K>, grid, dim3(WNW * 64), 0, ctx->stream, in, ll, det, det + P, det + 2 * P, ll_img,
                       tp, g);
    return 0;
}

template <int K>
int wav_level_synthesis(sbtv_ctx *ctx, const WavPlan &pl, int level, const double *ll, size_t ll_img, const double *det,
                        double *out, size_t out_img, int batch, const MomArgs *mom) {
    WavGeom g = wav_geom(pl, level);
    const size_t P = (size_t)pl.M * pl.N;
    g.img_in = (size_t)pl.bands() * P;
    g.img_out = out_img;
    WavTaps tp;
    for (int k = 0; k < 8; ++k) {
        tp.f0[k] = pl.f0[k];
        tp.f1[k] = pl.f1[k];
    }
    const dim3 grid = wav_grid_synthesis(pl, g, batch);
    if (mom)
        hipLaunchKernelGGL(wav_synthesis_moments_kernel<K>, grid, dim3(WNW * 64), 0, ctx->stream, ll, det, det + P, det + 2 * P,
                           ll_img, out, tp, g, *mom);
    else
        hipLaunchKernelGGL(wav_synthesis_kernel<K>, grid, dim3(WNW * 64), 0, ctx->stream, ll, det, det + P, det + 2 * P, ll_img,
                           out, tp, g);
    return 0;
}

template <int K>
int wav_lds_bytes(sbtv_ctx *ctx, int *analysis, int *synthesis) {
    hipFuncAttributes fa;
    SBTV_HIP(ctx, hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(wav_analysis_kernel<K>)));
    *analysis = (int)fa.sharedSizeBytes;
    SBTV_HIP(ctx, hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(wav_synthesis_kernel<K>)));
    *synthesis = (int)fa.sharedSizeBytes;
    return 0;
}

// what sbtv_diag_wavelet_geometry reports: wav_geom / wav_tiles and the tile constants exactly as the two launches above use
// them, and the static LDS of the two kernels as the loaded code object states it
int wav_report(sbtv_ctx *ctx, const WavPlan &pl, int level, int out[16]) {
    const WavGeom g = wav_geom(pl, level);
    out[0] = pl.J;
    out[1] = 1 << g.ls;
    out[2] = 1 << g.lq1;
    out[3] = 1 << g.lq2;
    out[4] = g.nr1;
    out[5] = g.nr2;
    out[6] = WT1;
    out[7] = WA_T2;
    out[8] = WS_T2;
    const dim3 ga = wav_grid_analysis(pl, g, 1), gs = wav_grid_synthesis(pl, g, 1);
    out[9] = (int)ga.x;
    out[10] = (int)ga.y;
    out[11] = (int)gs.y;
    out[12] = (pl.K - 1) << g.lq1;
    out[13] = (pl.K - 1) << g.lq2;
    switch (pl.K) {
        case 2: return wav_lds_bytes<2>(ctx, &out[14], &out[15]);
        case 4: return wav_lds_bytes<4>(ctx, &out[14], &out[15]);
        case 6: return wav_lds_bytes<6>(ctx, &out[14], &out[15]);
        default: return wav_lds_bytes<8>(ctx, &out[14], &out[15]);
    }
}

}  // namespace

int wav_plan(sbtv_ctx *ctx, int M, int N, const double *h, int hlen, int levels, bool orthonormal, WavPlan *pl) {
    if (!h) return fail(ctx, SBTV_ERR_BADARG, "wavelet: the scaling filter h is missing");
    if (hlen < 2 || hlen > 8 || (hlen & 1))
        return fail(ctx, SBTV_ERR_BADARG, "wavelet: the scaling filter must have an even length between 2 and 8");
    if (levels < 2) return fail(ctx, SBTV_ERR_BADARG, "wavelet: levels must be at least 2 (levels - 1 decomposition steps)");
    if (M < 1 || N < 1) return fail(ctx, SBTV_ERR_SIZE, "wavelet: empty image");
    const int J = levels - 1;
    // J first: the reach below is a shift by J - 1
    if (J > 30 || ((long long)(hlen - 1) << (J - 1)) >= (long long)(M < N ? M : N))
        return fail(ctx, SBTV_ERR_SIZE, "wavelet: (length(h) - 1) * 2^(levels - 2) must be smaller than both image dimensions");
    if (orthonormal) {
        double sum = 0.0;
        for (int k = 0; k < hlen; ++k) sum += h[k];
        bool ok = fabs(sum - sqrt(2.0)) <= 1e-10;
        for (int m = 0; ok && 2 * m < hlen; ++m) {
            double d = 0.0;
            for (int k = 0; k + 2 * m < hlen; ++k) d += h[k] * h[k + 2 * m];
            ok = fabs(d - (m == 0 ? 1.0 : 0.0)) <= 1e-10;
        }
        if (!ok) return fail(ctx, SBTV_ERR_BADARG, "wavelet: the scaling filter is not orthonormal (sum h = sqrt 2, unit norm, orthogonal to its even shifts)");
    }
    pl->M = M;
    pl->N = N;
    pl->K = hlen;
    pl->J = J;
    const double r = 1.0 / sqrt(2.0);
    for (int k = 0; k < 8; ++k) pl->f0[k] = pl->f1[k] = 0.0;
    for (int k = 0; k < hlen; ++k) {
        pl->f0[k] = h[k] * r;
        pl->f1[k] = ((k & 1) ? -1.0 : 1.0) * h[hlen - 1 - k] * r;
    }
    return 0;
}

// z[batch][3J+1][M N] <- W' x[batch][M N] (device pointers).  The approximation alternates between band 0 of z and a
// workspace image so that a_J lands in band 0.
int wav_analysis(sbtv_ctx *ctx, const WavPlan &pl, const double *x, double *z, int batch) {
    const size_t P = (size_t)pl.M * pl.N, zi = (size_t)pl.bands() * P;
    double *tmp = nullptr;
    if (pl.J > 1) SBTV_TRY(ws_get_t(ctx, "wav.tmp", P * batch, &tmp));
    const double *in = x;
    size_t in_img = P;
    for (int j = 1; j <= pl.J; ++j) {
        const bool to_z = ((pl.J - j) & 1) == 0;
        double *ll = to_z ? z : tmp;
        const size_t ll_img = to_z ? zi : P;
        double *det = z + (size_t)(1 + 3 * (j - 1)) * P;
        switch (pl.K) {
            case 2: SBTV_TRY(wav_level_analysis<2>(ctx, pl, j, in, in_img, ll, ll_img, det, batch)); break;
            case 4: SBTV_TRY(wav_level_analysis<4>(ctx, pl, j, in, in_img, ll, ll_img, det, batch)); break;
            case 6: SBTV_TRY(wav_level_analysis<6>(ctx, pl, j, in, in_img, ll, ll_img, det, batch)); break;
            default: SBTV_TRY(wav_level_analysis<8>(ctx, pl, j, in, in_img, ll, ll_img, det, batch)); break;
        }
        in = ll;
        in_img = ll_img;
    }
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

// x[batch][M N] <- W z[batch][3J+1][M N] (device pointers)
int wav_synthesis(sbtv_ctx *ctx, const WavPlan &pl, const double *z, double *x, int batch) {
    return wav_synthesis(ctx, pl, z, x, batch, nullptr);
}

// ... and, with mom (k > 0), the image as sample k of the moments: the level-1 launch (the one that stores x) accumulates
int wav_synthesis(sbtv_ctx *ctx, const WavPlan &pl, const double *z, double *x, int batch, const MomArgs *mom) {
    if (mom && (mom->k < 1 || !mom->mean || !mom->m2))
        return fail(ctx, SBTV_ERR_BADARG, "wav_synthesis: moments without a sample number or accumulators");
    const size_t P = (size_t)pl.M * pl.N, zi = (size_t)pl.bands() * P;
    double *tmp[2] = {nullptr, nullptr};
    if (pl.J > 1) SBTV_TRY(ws_get_t(ctx, "wav.tmp", P * batch, &tmp[0]));
    if (pl.J > 2) SBTV_TRY(ws_get_t(ctx, "wav.tmp2", P * batch, &tmp[1]));
    const double *ll = z;
    size_t ll_img = zi;
    for (int j = pl.J; j >= 1; --j) {
        double *out = (j == 1) ? x : tmp[j & 1];
        const double *det = z + (size_t)(1 + 3 * (j - 1)) * P;
        switch (pl.K) {
            case 2: SBTV_TRY(wav_level_synthesis<2>(ctx, pl, j, ll, ll_img, det, out, P, batch, j == 1 ? mom : nullptr)); break;
            case 4: SBTV_TRY(wav_level_synthesis<4>(ctx, pl, j, ll, ll_img, det, out, P, batch, j == 1 ? mom : nullptr)); break;
            case 6: SBTV_TRY(wav_level_synthesis<6>(ctx, pl, j, ll, ll_img, det, out, P, batch, j == 1 ? mom : nullptr)); break;
            default: SBTV_TRY(wav_level_synthesis<8>(ctx, pl, j, ll, ll_img, det, out, P, batch, j == 1 ? mom : nullptr)); break;
        }
        ll = out;
        ll_img = P;
    }
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_mrdwt_TI2D(sbtv_ctx *ctx, const double *x, int M, int N, int batch, const double *h, int hlen, int levels, double *z,
                    int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!x || !z || batch < 1) return fail(ctx, SBTV_ERR_BADARG, "mrdwt_TI2D: missing required argument");
    WavPlan pl;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, false, &pl));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)M * N, nx = P * batch, nz = nx * pl.bands();
    const double *xd = nullptr;
    double *zd = nullptr;
    SBTV_TRY(stage_in(ctx, "wav.in", x, nx, flags, &xd));
    SBTV_TRY(stage_out_buf(ctx, "wav.out", z, nz, flags, &zd));
    SBTV_TRY(wav_analysis(ctx, pl, xd, zd, batch));
    SBTV_TRY(stage_out_copy(ctx, z, zd, nz, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->calls += batch;
    return canary_epilogue(ctx, 0);
}

int sbtv_mirdwt_TI2D(sbtv_ctx *ctx, const double *z, int M, int N, int batch, const double *h, int hlen, int levels, double *x,
                     int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!x || !z || batch < 1) return fail(ctx, SBTV_ERR_BADARG, "mirdwt_TI2D: missing required argument");
    WavPlan pl;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, false, &pl));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)M * N, nx = P * batch, nz = nx * pl.bands();
    const double *zd = nullptr;
    double *xd = nullptr;
    SBTV_TRY(stage_in(ctx, "wav.in", z, nz, flags, &zd));
    SBTV_TRY(stage_out_buf(ctx, "wav.out", x, nx, flags, &xd));
    SBTV_TRY(wav_synthesis(ctx, pl, zd, xd, batch));
    SBTV_TRY(stage_out_copy(ctx, x, xd, nx, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->calls += batch;
    return canary_epilogue(ctx, 0);
}

int sbtv_soft(sbtv_ctx *ctx, const double *x, int M, int N, int batch, const double *T, double *out, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!x || !out || !T || batch < 1 || M < 1 || N < 1) return fail(ctx, SBTV_ERR_BADARG, "soft: missing required argument");
    for (int b = 0; b < batch; ++b)
        if (!(T[b] >= 0.0)) return fail(ctx, SBTV_ERR_BADARG, "soft: the threshold must be non-negative");
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)M * N, n = P * batch;
    const double *xd = nullptr;
    double *od = nullptr, *Td = nullptr;
    SBTV_TRY(stage_in(ctx, "wav.in", x, n, flags, &xd));
    SBTV_TRY(stage_out_buf(ctx, "wav.out", out, n, flags, &od));
    SBTV_TRY(ws_get_t(ctx, "wav.T", (size_t)batch, &Td));
    SBTV_HIP(ctx, hipMemcpyAsync(Td, T, sizeof(double) * batch, hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    size_t nb = (P + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(wav_soft_kernel, dim3((unsigned)nb, (unsigned)batch), dim3(256), 0, ctx->stream, xd, (const double *)Td, od, P);
    SBTV_HIP(ctx, hipGetLastError());
    SBTV_TRY(stage_out_copy(ctx, out, od, n, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

int sbtv_diag_wavelet_geometry(sbtv_ctx *ctx, int M, int N, int hlen, int levels, int level, int out[16]) {
    if (!ctx || !out) return SBTV_ERR_BADARG;
    static const double h[8] = {0.0};                                     // wav_plan reads it after its checks only
    WavPlan pl;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, false, &pl));
    if (level < 1 || level > pl.J) return fail(ctx, SBTV_ERR_BADARG, "diag_wavelet_geometry: the level must lie in 1..levels - 1");
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    return wav_report(ctx, pl, level, out);
}

}  // extern "C"

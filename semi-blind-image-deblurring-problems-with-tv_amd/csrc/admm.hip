// The two other ADMM front-ends of the SALSA toolbox that call the Chambolle TV prox, built from
// the same device kernels as SALSA_v2:
//   C-SALSA  (SALSA/CSALSA_v2.m:160-561)  min TV(x)  s.t. ||Ax - y|| <= epsilon
//   CoRAL    (SALSA/CoRAL_v2.m:2-476)     min 0.5||Ax-y||^2 + tau1 TV(x) + tau2 TV(x)   (two split copies)
// and the masked-observation SALSA (no counterpart in the reference: SALSA/SALSA.m:103-104,308-312,463-464 takes a mask OR a
// blur), min 0.5 sum(m .* (Bx - y).^2) + tau TV(x) with the splits u = x and v = Bx (masked_one below).
// Neither is called by the reference's demos, so they are not fused to the last pass; what they share with the SALSA
// loop since round 3 is its stream discipline: the Chambolle launches of an outer iteration are OPTIMISTIC (all TViters
// iterations back to back, no stop-rule kernels, no redo pass; the host applies chambolle_prox_TV_stop.m:131 to the step
// sums it reads with the iteration's scalars and, should the rule ever fire before the last step, repeats the solve with
// exact launches), and the host evaluates the outer stop rule one iteration late while the next iteration already runs
// (x is double-buffered, so the result of the stopping iteration is intact).  The images of a batch are solved one after
// another.
#include <chrono>
#include <cmath>

#include "sbtv_internal.h"

#pragma clang fp contract(off)

namespace sbtv {

namespace {

constexpr int AB = 256;

__device__ __forceinline__ double ad_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// block-reduce NQ running sums and store them as partials[q * gridDim.x + blockIdx.x]
template <int NQ>
__device__ __forceinline__ void ad_store_partials(double (&acc)[NQ], double *__restrict__ partials) {
    __shared__ double red[NQ * 4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        const double a = ad_wave_sum(acc[c]);
        if (lane == 0) red[c * 4 + w] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NQ; ++c)
            partials[(size_t)c * gridDim.x + blockIdx.x] = (red[c * 4] + red[c * 4 + 1]) + (red[c * 4 + 2] + red[c * 4 + 3]);
    }
}

#define AD_LOOP(q, P) for (size_t q = (size_t)blockIdx.x * AB + threadIdx.x; q < (P) / 2; q += (size_t)gridDim.x * AB)
#define AD_LD(p, q) (*reinterpret_cast<const double2 *>((p) + 2 * (q)))
#define AD_ST(p, q, v) (*reinterpret_cast<double2 *>((p) + 2 * (q)) = (v))

// g = x - b
__global__ __launch_bounds__(AB) void ad_sub_kernel(const double *__restrict__ x, const double *__restrict__ b,
                                                     double *__restrict__ g, size_t P) {
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), bv = AD_LD(b, q);
        AD_ST(g, q, make_double2(xv.x - bv.x, xv.y - bv.y));
    }
}

// ---- C-SALSA -----------------------------------------------------------------------------------
// w = mu2 * (y + v + bv)                                                   (CSALSA_v2.m:467)
__global__ __launch_bounds__(AB) void csalsa_w_kernel(const double *__restrict__ y, const double *__restrict__ v,
                                                       const double *__restrict__ bv, const double *__restrict__ par,
                                                       double *__restrict__ w, size_t P) {
    const double mu2 = par[1];
    AD_LOOP(q, P) {
        const double2 a = AD_LD(y, q), b = AD_LD(v, q), c = AD_LD(bv, q);
        AD_ST(w, q, make_double2(mu2 * ((a.x + b.x) + c.x), mu2 * ((a.y + b.y) + c.y)));
    }
}

// partials[nb] = sum (Ax - y - bv)^2                                        (:483-484)
__global__ __launch_bounds__(AB) void csalsa_ve_kernel(const double *__restrict__ Ax, const double *__restrict__ y,
                                                        const double *__restrict__ bv, double *__restrict__ partials,
                                                        size_t P) {
    double acc[1] = {0.0};
    AD_LOOP(q, P) {
        const double2 a = AD_LD(Ax, q), b = AD_LD(y, q), c = AD_LD(bv, q);
        const double e0 = (a.x - b.x) - c.x, e1 = (a.y - b.y) - c.y;
        acc[0] += e0 * e0 + e1 * e1;
    }
    ad_store_partials<1>(acc, partials);
}

// projection of ve on the epsilon ball, multiplier updates and the sums of the traces (:483-501,534)
//   partials [6][nb]: (Ax-y)^2, (Ax-y-v)^2, (x-u)^2, (x-true)^2, (x-xprev)^2, x^2
__global__ __launch_bounds__(AB) void csalsa_update_kernel(const double *__restrict__ Ax, const double *__restrict__ y,
                                                            const double *__restrict__ x, const double *__restrict__ u,
                                                            double *__restrict__ v, double *__restrict__ bv,
                                                            double *__restrict__ bu, const double *__restrict__ tru,
                                                            const double *__restrict__ xprev,
                                                            const double *__restrict__ nve2, double eps,
                                                            double *__restrict__ partials, size_t P) {
    const double n_ve = sqrt(nve2[0]);
    const bool inside = n_ve <= eps;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    AD_LOOP(q, P) {
        const double2 a = AD_LD(Ax, q), yy = AD_LD(y, q), c = AD_LD(bv, q);
        const double t0 = a.x - yy.x, t1 = a.y - yy.y;
        const double e0 = t0 - c.x, e1 = t1 - c.y;
        const double v0 = inside ? e0 : e0 / n_ve * eps, v1 = inside ? e1 : e1 / n_ve * eps;
        AD_ST(v, q, make_double2(v0, v1));
        const double r0 = t0 - v0, r1 = t1 - v1;
        AD_ST(bv, q, make_double2(c.x - r0, c.y - r1));
        const double2 xv = AD_LD(x, q), uv = AD_LD(u, q), bb = AD_LD(bu, q);
        const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
        AD_ST(bu, q, make_double2(bb.x - d0, bb.y - d1));
        acc[0] += t0 * t0 + t1 * t1;
        acc[1] += r0 * r0 + r1 * r1;
        acc[2] += d0 * d0 + d1 * d1;
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[3] += m0 * m0 + m1 * m1;
        }
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[4] += m0 * m0 + m1 * m1;
        }
        acc[5] += xv.x * xv.x + xv.y * xv.y;
    }
    ad_store_partials<6>(acc, partials);
}

// ---- C-SALSA with the constraint split kept as a spectrum (default; see csalsa_one) ------------------------------
// After the row pass: the three spectral sums of the iteration -> the projection factor s = min(1, eps / ||ve||), the
// coefficients of the next row pass and the two traces that depend on Ax.  st: [0] mu2, [1] c_e = mu2 (2s-1),
// [2] c_keep = 1-s, [3] sum |E|^2 of the previous iteration (unscaled), [4] 1 - s of the previous iteration.
//   out[0] = ||Ax-y||^2, out[1] = ||Ax-y-v||^2 = ||(1-s) E' - (1-s_prev) E||^2 from |E'|^2, |E|^2 and |E'-E|^2:
//   (a-c)(a A1 - c A1p) + a c A2 (no difference of large numbers once the iteration settles: a -> c, E' -> E)
__global__ __launch_bounds__(256) void csalsa_scal_kernel(const double *__restrict__ accp, int nrb, double *__restrict__ st,
                                                          double eps, double pv, double *__restrict__ out) {
    // the three sums of the row pass, partials [3][nrb], in the order of reduce_partials_kernel
    __shared__ double red[4 * 3], tot[3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int i = threadIdx.x; i < nrb; i += 256) s += accp[(size_t)c * nrb + i];
        s = ad_wave_sum(s);
        if (lane == 0) red[c * 4 + w] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3) tot[threadIdx.x] = (red[threadIdx.x * 4] + red[threadIdx.x * 4 + 1]) + (red[threadIdx.x * 4 + 2] + red[threadIdx.x * 4 + 3]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double A0 = tot[0], A1 = tot[1], A2 = tot[2];
    const double n_ve = sqrt(A1 * pv);
    const double sfac = (n_ve <= eps) ? 1.0 : eps / n_ve;
    const double a = 1.0 - sfac, c = st[4], A1p = st[3];
    const double d1 = ((a - c) * (a * A1 - c * A1p) + a * c * A2) * pv;
    out[0] = A0 * pv;
    out[1] = d1 > 0.0 ? d1 : 0.0;
    st[1] = st[0] * (2.0 * sfac - 1.0);
    st[2] = a;
    st[3] = A1;
    st[4] = a;
}

// after the prox: bu <- bu - (x - u) (:492) and the sums of the traces that live in the image domain
//   partials [5][nb]: (x-u)^2, (x-true)^2, (x-xprev)^2, x^2, periodic TV(x) (utils/TVnorm.m:2)
__global__ __launch_bounds__(AB) void csalsa_post_kernel(const double *__restrict__ x, const double *__restrict__ u,
                                                          double *__restrict__ bu, const double *__restrict__ tru,
                                                          const double *__restrict__ xprev, double *__restrict__ partials,
                                                          unsigned M, unsigned N, size_t P) {
    double acc[5] = {0, 0, 0, 0, 0};
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), uv = AD_LD(u, q), bb = AD_LD(bu, q);
        const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
        AD_ST(bu, q, make_double2(bb.x - d0, bb.y - d1));
        acc[0] += d0 * d0 + d1 * d1;
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[1] += m0 * m0 + m1 * m1;
        }
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[2] += m0 * m0 + m1 * m1;
        }
        acc[3] += xv.x * xv.x + xv.y * xv.y;
        // element 2q = (i, j), i even (M is even on this path): left neighbours in column j-1, upper neighbour of row i
        const unsigned idx = (unsigned)(2 * q), j = idx / M, i = idx - j * M;
        const size_t lcol = (size_t)(j > 0 ? j - 1 : N - 1) * M + i;
        const double2 xl = *reinterpret_cast<const double2 *>(x + lcol);
        const double xu = x[(size_t)j * M + (i > 0 ? i - 1 : M - 1)];
        const double h0 = xv.x - xl.x, v0 = xv.x - xu, h1 = xv.y - xl.y, v1 = xv.y - xv.x;
        acc[4] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
    }
    ad_store_partials<5>(acc, partials);
}

// ---- CoRAL -------------------------------------------------------------------------------------
// s = (mu1 (u+bu) + mu2 (v+bv)) / mu_ls                                     (CoRAL_v2.m:411, ATy enters spectrally)
// TVS: also the periodic TV norms of u and v (utils/TVnorm.m:2) for the objective (:425), partials [2][nb]: the two
// arrays are in flight here anyway (M even; element 2q = (i, j) with i even)
template <bool TVS>
__global__ __launch_bounds__(AB) void coral_s_kernel(const double *__restrict__ u, const double *__restrict__ bu,
                                                      const double *__restrict__ v, const double *__restrict__ bv,
                                                      double mu1, double mu2, double mu_ls, double *__restrict__ s,
                                                      double *__restrict__ partials, unsigned M, unsigned N, size_t P) {
    double acc[2] = {0, 0};
    AD_LOOP(q, P) {
        const double2 a = AD_LD(u, q), b = AD_LD(bu, q), c = AD_LD(v, q), d = AD_LD(bv, q);
        AD_ST(s, q, make_double2((mu1 * (a.x + b.x) + mu2 * (c.x + d.x)) / mu_ls,
                                 (mu1 * (a.y + b.y) + mu2 * (c.y + d.y)) / mu_ls));
        if constexpr (TVS) {
            const unsigned idx = (unsigned)(2 * q), j = idx / M, i = idx - j * M;
            const size_t lcol = (size_t)(j > 0 ? j - 1 : N - 1) * M + i, up = (size_t)j * M + (i > 0 ? i - 1 : M - 1);
            const double2 ul = *reinterpret_cast<const double2 *>(u + lcol), vl = *reinterpret_cast<const double2 *>(v + lcol);
            const double uu = u[up], vu = v[up];
            {
                const double h0 = a.x - ul.x, v0 = a.x - uu, h1 = a.y - ul.y, v1 = a.y - a.x;
                acc[0] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
            }
            {
                const double h0 = c.x - vl.x, v0 = c.x - vu, h1 = c.y - vl.y, v1 = c.y - c.x;
                acc[1] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
            }
        }
    }
    if constexpr (TVS) ad_store_partials<2>(acc, partials);
}

// bu += u - x ; bv += v - x ; g1 = x - bu ; g2 = x - bv  (:420-421 and the next prox inputs :401,406)
//   partials [7][nb]: (x-true)^2, (x-u)^2, (x-v)^2, x^2, u^2, v^2, (x-xprev)^2
__global__ __launch_bounds__(AB) void coral_post_kernel(const double *__restrict__ x, const double *__restrict__ xprev,
                                                         const double *__restrict__ u, const double *__restrict__ v,
                                                         double *__restrict__ bu, double *__restrict__ bv,
                                                         double *__restrict__ g1, double *__restrict__ g2,
                                                         const double *__restrict__ tru, double *__restrict__ partials,
                                                         size_t P) {
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), uv = AD_LD(u, q), vv = AD_LD(v, q);
        double2 b1 = AD_LD(bu, q), b2 = AD_LD(bv, q);
        b1.x = b1.x + (uv.x - xv.x);
        b1.y = b1.y + (uv.y - xv.y);
        b2.x = b2.x + (vv.x - xv.x);
        b2.y = b2.y + (vv.y - xv.y);
        AD_ST(bu, q, b1);
        AD_ST(bv, q, b2);
        AD_ST(g1, q, make_double2(xv.x - b1.x, xv.y - b1.y));
        AD_ST(g2, q, make_double2(xv.x - b2.x, xv.y - b2.y));
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[0] += m0 * m0 + m1 * m1;
        }
        {
            const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
            acc[1] += d0 * d0 + d1 * d1;
            const double e0 = xv.x - vv.x, e1 = xv.y - vv.y;
            acc[2] += e0 * e0 + e1 * e1;
        }
        acc[3] += xv.x * xv.x + xv.y * xv.y;
        acc[4] += uv.x * uv.x + uv.y * uv.y;
        acc[5] += vv.x * vv.x + vv.y * vv.y;
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[6] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<7>(acc, partials);
}

// ---- masked-observation SALSA (masked_one) ------------------------------------------------------
// w = m .* y: the right-hand side of the start x = B'(m .* y) ('INITIALIZATION' 2)
__global__ __launch_bounds__(AB) void masked_my_kernel(const double *__restrict__ m, const double *__restrict__ y,
                                                        double *__restrict__ w, size_t P) {
    AD_LOOP(q, P) {
        const double2 mv = AD_LD(m, q), yv = AD_LD(y, q);
        AD_ST(w, q, make_double2(mv.x * yv.x, mv.y * yv.y));
    }
}

// The one element-wise pass of an outer iteration, after the two inverse transforms (x, Bx) and with this iteration's u and v:
//   bu += u - x ; bv += v - Bx ; g = x - bu (the next prox input) ; v <- (m .* y + mu2 (Bx - bv)) ./ (m + mu2) (the next v)
//   partials [9 or 10][nb]: m (Bx-y)^2, (x-u)^2, (Bx-v)^2, x^2, u^2, Bx^2, v^2, (x-true)^2, (x-xprev)^2 and, TVS, the periodic
//   TV norm of u (utils/TVnorm.m:2; M even, element 2q = (i, j) with i even), all with the v this iteration solved with
template <bool TVS>
__global__ __launch_bounds__(AB) void masked_post_kernel(const double *__restrict__ x, const double *__restrict__ xprev,
                                                          const double *__restrict__ Bx, const double *__restrict__ u,
                                                          const double *__restrict__ y, const double *__restrict__ m,
                                                          double *__restrict__ bu, double *__restrict__ v,
                                                          double *__restrict__ bv, double *__restrict__ g,
                                                          const double *__restrict__ tru, double mu2,
                                                          double *__restrict__ partials, unsigned M, unsigned N, size_t P) {
    constexpr int NQ = TVS ? 10 : 9;
    double acc[NQ];
#pragma unroll
    for (int c = 0; c < NQ; ++c) acc[c] = 0.0;
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), ax = AD_LD(Bx, q), uv = AD_LD(u, q), vv = AD_LD(v, q);
        const double2 yv = AD_LD(y, q), mv = AD_LD(m, q);
        double2 b1 = AD_LD(bu, q), b2 = AD_LD(bv, q);
        b1.x = b1.x + (uv.x - xv.x);
        b1.y = b1.y + (uv.y - xv.y);
        b2.x = b2.x + (vv.x - ax.x);
        b2.y = b2.y + (vv.y - ax.y);
        AD_ST(bu, q, b1);
        AD_ST(bv, q, b2);
        AD_ST(g, q, make_double2(xv.x - b1.x, xv.y - b1.y));
        AD_ST(v, q, make_double2((mv.x * yv.x + mu2 * (ax.x - b2.x)) / (mv.x + mu2),
                                 (mv.y * yv.y + mu2 * (ax.y - b2.y)) / (mv.y + mu2)));
        {
            const double e0 = ax.x - yv.x, e1 = ax.y - yv.y;
            acc[0] += mv.x * (e0 * e0) + mv.y * (e1 * e1);
            const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
            acc[1] += d0 * d0 + d1 * d1;
            const double r0 = ax.x - vv.x, r1 = ax.y - vv.y;
            acc[2] += r0 * r0 + r1 * r1;
        }
        acc[3] += xv.x * xv.x + xv.y * xv.y;
        acc[4] += uv.x * uv.x + uv.y * uv.y;
        acc[5] += ax.x * ax.x + ax.y * ax.y;
        acc[6] += vv.x * vv.x + vv.y * vv.y;
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[7] += m0 * m0 + m1 * m1;
        }
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[8] += m0 * m0 + m1 * m1;
        }
        if constexpr (TVS) {
            const unsigned idx = (unsigned)(2 * q), j = idx / M, i = idx - j * M;
            const size_t lcol = (size_t)(j > 0 ? j - 1 : N - 1) * M + i;
            const double2 ul = *reinterpret_cast<const double2 *>(u + lcol);
            const double uu = u[(size_t)j * M + (i > 0 ? i - 1 : M - 1)];
            const double h0 = uv.x - ul.x, v0 = uv.x - uu, h1 = uv.y - ul.y, v1 = uv.y - uv.x;
            acc[NQ - 1] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
        }
    }
    ad_store_partials<NQ>(acc, partials);
}

// ---- wavelet-l1 SALSA (wavelet_one) -------------------------------------------------------------------------------
// l1 norm of the start xw and its distance to the true coefficients: partials [2][nb]
__global__ __launch_bounds__(AB) void wav_init_kernel(const double *__restrict__ xw, const double *__restrict__ tru,
                                                       double *__restrict__ partials, size_t C) {
    double acc[2] = {0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 v = AD_LD(xw, q);
        acc[0] += fabs(v.x) + fabs(v.y);
        if (tru) {
            const double2 t = AD_LD(tru, q);
            const double m0 = v.x - t.x, m1 = v.y - t.y;
            acc[1] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<2>(acc, partials);
}

// The prox of an outer iteration on the state (s, we) of the previous one, xw = s + we and bu = -we:
//   u = soft(xw - bu, T) = soft(s + 2 we, T) ; s' = u + bu = u - we ; partials [2][nb]: |u|, u^2
__global__ __launch_bounds__(AB) void wav_prox_kernel(const double *__restrict__ s, const double *__restrict__ we,
                                                       double *__restrict__ sn, double T, double *__restrict__ partials,
                                                       size_t C) {
    double acc[2] = {0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 sv = AD_LD(s, q), wv = AD_LD(we, q);
        const double u0 = wav_soft(sv.x + 2.0 * wv.x, T), u1 = wav_soft(sv.y + 2.0 * wv.y, T);
        AD_ST(sn, q, make_double2(u0 - wv.x, u1 - wv.y));
        acc[0] += fabs(u0) + fabs(u1);
        acc[1] += u0 * u0 + u1 * u1;
    }
    ad_store_partials<2>(acc, partials);
}

// After the analysis we' = W'(xi - z) of an outer iteration: xw' = s' + we', u = s' + we (we: the previous iteration's), so
// xw' - u = we' - we.  partials [4][nb]: (xw'-u)^2, xw'^2, (xw'-true)^2, (xw'-xw)^2 with xw = s + we (sp == null: not summed)
__global__ __launch_bounds__(AB) void wav_post_kernel(const double *__restrict__ sn, const double *__restrict__ wn,
                                                       const double *__restrict__ we, const double *__restrict__ sp,
                                                       const double *__restrict__ tru, double *__restrict__ partials,
                                                       size_t C) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 sv = AD_LD(sn, q), wv = AD_LD(wn, q), wo = AD_LD(we, q);
        const double x0 = sv.x + wv.x, x1 = sv.y + wv.y;
        const double d0 = wv.x - wo.x, d1 = wv.y - wo.y;
        acc[0] += d0 * d0 + d1 * d1;
        acc[1] += x0 * x0 + x1 * x1;
        if (tru) {
            const double2 t = AD_LD(tru, q);
            const double m0 = x0 - t.x, m1 = x1 - t.y;
            acc[2] += m0 * m0 + m1 * m1;
        }
        if (sp) {
            const double2 so = AD_LD(sp, q);
            const double m0 = x0 - (so.x + wo.x), m1 = x1 - (so.y + wo.y);
            acc[3] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<4>(acc, partials);
}

// xw = s + we
__global__ __launch_bounds__(AB) void wav_sum_kernel(const double *__restrict__ s, const double *__restrict__ we,
                                                      double *__restrict__ xw, size_t C) {
    AD_LOOP(q, C) {
        const double2 sv = AD_LD(s, q), wv = AD_LD(we, q);
        AD_ST(xw, q, make_double2(sv.x + wv.x, sv.y + wv.y));
    }
}

// ---- analysis-prior wavelet SALSA (analysis_one) ------------------------------------------------------------------
// The one coefficient pass of an outer iteration k, after the analysis w = W'x_k, on the state (s, bu) = (u_k + bu_{k-1}, bu_{k-1}):
//   u = s - bu (exactly zero where the threshold cut it: there s == bu bit for bit) ; bu' = bu + (u - w)    (SALSA_v2.m:440)
//   u' = soft(w - bu', T) ; s' = u' + bu'                                                                  (:431 of k + 1)
//   partials [4][nb]: |u|, u^2, (w-u)^2, w^2
// The start is the same pass with s = w_0 and bu = 0.
__global__ __launch_bounds__(AB) void wav_astep_kernel(const double *__restrict__ s, const double *__restrict__ bu,
                                                        const double *__restrict__ w, double *__restrict__ bun,
                                                        double *__restrict__ sn, double T, double *__restrict__ partials,
                                                        size_t C) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 sv = AD_LD(s, q), bv = AD_LD(bu, q), wv = AD_LD(w, q);
        const double u0 = sv.x - bv.x, u1 = sv.y - bv.y;
        const double d0 = wv.x - u0, d1 = wv.y - u1;
        const double b0 = bv.x + (u0 - wv.x), b1 = bv.y + (u1 - wv.y);
        AD_ST(bun, q, make_double2(b0, b1));
        AD_ST(sn, q, make_double2(wav_soft(wv.x - b0, T) + b0, wav_soft(wv.y - b1, T) + b1));
        acc[0] += fabs(u0) + fabs(u1);
        acc[1] += u0 * u0 + u1 * u1;
        acc[2] += d0 * d0 + d1 * d1;
        acc[3] += wv.x * wv.x + wv.y * wv.y;
    }
    ad_store_partials<4>(acc, partials);
}

// the image-domain sums of an outer iteration: partials [3][nb]: (x-true)^2, (x-xprev)^2, x^2 (tru / xprev null: not summed)
__global__ __launch_bounds__(AB) void ad_xsums_kernel(const double *__restrict__ x, const double *__restrict__ tru,
                                                       const double *__restrict__ xprev, double *__restrict__ partials,
                                                       size_t P) {
    double acc[3] = {0.0, 0.0, 0.0};
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q);
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[0] += m0 * m0 + m1 * m1;
        }
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[1] += m0 * m0 + m1 * m1;
        }
        acc[2] += xv.x * xv.x + xv.y * xv.y;
    }
    ad_store_partials<3>(acc, partials);
}

// ---- wavelet-l1 FISTA (fista_l1_one) ------------------------------------------------------------------------------
// zy = zx + c (zx - zxo): the image W y of the momentum point y = x + c (x - xo), by linearity of W
__global__ __launch_bounds__(AB) void fl1_momentum_kernel(const double *__restrict__ zx, const double *__restrict__ zxo,
                                                           double c, double *__restrict__ zy, size_t P) {
    AD_LOOP(q, P) {
        const double2 a = AD_LD(zx, q), b = AD_LD(zxo, q);
        AD_ST(zy, q, make_double2(a.x + c * (a.x - b.x), a.y + c * (a.y - b.y)));
    }
}

// The step of an iteration (my_fista_l1.m:38-39,42 of the iteration before): y = x + c (x - xo) ; xn = soft(y - (1/L) g, T),
// T = tau / L, written over xo.  partials [3 or 4][nb]: |xn|, xn^2, (xn - x)^2 and, TRU, (xn - true)^2
template <bool TRU>
__global__ __launch_bounds__(AB) void fl1_step_kernel(const double *__restrict__ x, double *__restrict__ xo,
                                                       const double *__restrict__ g, const double *__restrict__ tru, double c,
                                                       double invL, double T, double *__restrict__ partials, size_t C) {
    constexpr int NQ = TRU ? 4 : 3;
    double acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = 0.0;
    AD_LOOP(q, C) {
        const double2 xv = AD_LD(x, q), ov = AD_LD(xo, q), gv = AD_LD(g, q);
        const double y0 = xv.x + c * (xv.x - ov.x), y1 = xv.y + c * (xv.y - ov.y);
        const double n0 = wav_soft(y0 - invL * gv.x, T), n1 = wav_soft(y1 - invL * gv.y, T);
        AD_ST(xo, q, make_double2(n0, n1));
        acc[0] += fabs(n0) + fabs(n1);
        acc[1] += n0 * n0 + n1 * n1;
        const double d0 = n0 - xv.x, d1 = n1 - xv.y;
        acc[2] += d0 * d0 + d1 * d1;
        if constexpr (TRU) {
            const double2 t = AD_LD(tru, q);
            const double m0 = n0 - t.x, m1 = n1 - t.y;
            acc[3] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<NQ>(acc, partials);
}

inline int ad_blocks(size_t P) {
    size_t nb = (P / 2 + AB - 1) / AB;
    if (nb > 1024) nb = 1024;
    return nb < 1 ? 1 : (int)nb;
}

// everything one single-image solve shares: the operator layer "admm" with the spectra of the PSF and (yd given) of y
int admm_common(sbtv_ctx *ctx, int M, int N, const double *taps, int taille, const double *yd, BlurOp *c) {
    SBTV_TRY(check_even_pixels(ctx, M, N));
    SBTV_TRY(op_open(ctx, "admm", M, N, 1, "Y", c));
    double *taps_d = nullptr;
    SBTV_TRY(ws_get_t(ctx, "admm.taps", (size_t)taille * taille, &taps_d));
    SBTV_HIP(ctx, hipMemcpyAsync(taps_d, taps, sizeof(double) * taille * taille, hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SBTV_TRY(psf_spectrum(ctx, c->fp, taps_d, taille, c->Hs));
    if (yd) SBTV_TRY(op_spectrum(ctx, c->fp, yd, nullptr, c->S, c->Ys));
    return 0;
}

// C-SALSA: the constraint split (v, bv) as ONE spectrum and a scalar (default) or as images (SBTV_CSALSA_SPECTRAL=0)
inline bool csalsa_spectral_wanted() {
    static const bool on = [] {
        const char *e = getenv("SBTV_CSALSA_SPECTRAL");
        return !(e && e[0] == '0');
    }();
    return on;
}

// the four doubles of "admm.par" (each driver says what they are), on the device before anything is enqueued that reads them
int upload_par(sbtv_ctx *ctx, double *par, const double (&h)[4]) {
    SBTV_HIP(ctx, hipMemcpyAsync(par, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// The warm-started TV prox of an outer iteration: a plan (of one image, or of CoRAL's two), its threshold(s) `lam` on the
// device and K iterations per prox.
struct AdmmProx {
    ProxPlan pp;
    const double *lam = nullptr;
    int K = 0;
    double tol = 0.0, tau = 0.0;
    long long nlaunch = 0;       // optimistic launches so far: the kernels read dual buffer cur ^ (nlaunch & 1)

    int plan(sbtv_ctx *ctx, int M, int N, int batch, const char *tag, int iters, const sbtv_salsa_opts *opts) {
        K = iters;
        tol = opts->chambolle_tol;
        tau = opts->chambolle_tau;
        return prox_plan(ctx, M, N, batch, &pp, tag);
    }
    // arms the control block(s); fresh: before the first prox, on zero duals
    int arm(sbtv_ctx *ctx, bool fresh) { return prox_reset(ctx, pp, lam, 1.0, K, tol, tau, !fresh, nullptr); }
    // f = prox(g).  Exact: re-armed, the kernels apply the stop rule.  Optimistic: all K iterations back to back on the
    // control block as `arm` left it, and the step sums of the K iterations (of image b at stepsums + b FSTRIDE) for the
    // host's rule: reduced at once, or with a job list together with the other sums of the iteration
    int run(sbtv_ctx *ctx, const double *g, double *f, bool optimistic, double *stepsums, RedJobs *jb) {
        if (!optimistic) {
            SBTV_TRY(arm(ctx, false));
            return prox_iterate(ctx, pp, g, K, f);
        }
        SBTV_TRY(prox_iterate(ctx, pp, g, K, f, false, 1, (int)(nlaunch & 1), nullptr));
        nlaunch += prox_launches(pp, K);
        const int nvec = (pp.batch - 1) * FSTRIDE + K;
        if (!jb) return reduce_partials(ctx, pp.partials, nvec, pp.fnblk, stepsums);
        jb->add(pp.partials, nvec, pp.fnblk, stepsums);
        return 0;
    }
    // the host's rule on the step sums of an optimistic prox (SOLVE_RESTART_EXACT: it fired early)
    int check(sbtv_ctx *ctx, const double *stepsums) { return spec_stop_rule(ctx, pp, stepsums, K, tol); }
};

// What a solve carries through its pipelined loop.  Per-iteration scalars travel through two pinned slots; an event per
// slot tells the host (which runs one iteration ahead) when the slot of an iteration holds its scalars.  Beside them: the
// clock of `times`, the operator counts, the Chambolle iterations of sbtv_last_timing.
struct AdmmRun {
    static constexpr int NSUM = 94;                // doubles per slot, then the iteration counts of up to two exact proxes
    sbtv_ctx *ctx = nullptr;
    double *hs[2] = {nullptr, nullptr};            // the two slots (pinned): the sums ...
    int *khs[2] = {nullptr, nullptr};              // ... and the counts, at [0] and [2]
    hipEvent_t ev[2] = {nullptr, nullptr};
    long long opt_iters[2] = {0, 0};
    std::chrono::steady_clock::time_point t0;
    int numA = 0, numAt = 0;
    long long prox_iters = 0;
    int *numA_out = nullptr, *numAt_out = nullptr, *n_outer_out = nullptr;

    ~AdmmRun() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int open(sbtv_ctx *c, int *numA_o, int *numAt_o, int *n_outer_o) {
        ctx = c;
        numA_out = numA_o;
        numAt_out = numAt_o;
        n_outer_out = n_outer_o;
        PinnedLayout lay;
        PinnedField<double> fs[2];
        PinnedField<int> fk[2];
        for (int s = 0; s < 2; ++s) {
            fs[s] = lay.add<double>(NSUM);
            fk[s] = lay.add<int>(4);
        }
        void *pz = nullptr;
        SBTV_TRY(pinned_get(ctx, lay.bytes(), &pz));
        for (int s = 0; s < 2; ++s) {
            hs[s] = fs[s].at(pz);
            khs[s] = fk[s].at(pz);
        }
        for (auto &e : ev) SBTV_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return 0;
    }
    // the loop begins: sbtv_last_timing and `times` count from here
    int start() {
        t0 = std::chrono::steady_clock::now();
        SBTV_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
        return 0;
    }
    // before the loop: the first n doubles of `sums`, read back through slot 0
    int fetch(const double *sums, int n, const double **h) {
        SBTV_HIP(ctx, hipMemcpyAsync(hs[0], sums, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *h = hs[0];
        return 0;
    }
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    // end of enqueue(outer): the first n doubles of `sums` into the iteration's slot.  Its Chambolle iterations are `iters` if
    // its proxes were optimistic; exact ones hand the control blocks that count theirs (k0, k1: device)
    int publish(int outer, const double *sums, int n, long long iters, const ProxCtrl *k0 = nullptr,
                const ProxCtrl *k1 = nullptr) {
        double *hsl = hs[outer & 1];
        int *kh = khs[outer & 1];
        kh[0] = kh[2] = 0;
        opt_iters[outer & 1] = iters;
        SBTV_HIP(ctx, hipGetLastError());
        SBTV_HIP(ctx, hipMemcpyAsync(hsl, sums, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        if (k0) SBTV_HIP(ctx, hipMemcpyAsync(kh, &k0->k, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (k1) SBTV_HIP(ctx, hipMemcpyAsync(kh + 2, &k1->k, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        SBTV_HIP(ctx, hipEventRecord(ev[outer & 1], ctx->stream));
        return 0;
    }
    // head of process(outer): waits for the iteration's slot, books its Chambolle iterations
    int wait(int outer, const double **hsl) {
        *hsl = hs[outer & 1];
        SBTV_HIP(ctx, hipEventSynchronize(ev[outer & 1]));
        const int *kh = khs[outer & 1];
        prox_iters += opt_iters[outer & 1] + kh[0] + kh[2];
        return 0;
    }
    // after the loop: its device time (sbtv_last_timing), the result x (null: the caller fetches its own), the counters
    int finish(size_t P, int last, const double *x, double *x_out) {
        SBTV_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SBTV_TRY(loop_timing(ctx, 0.0, prox_iters, 1, P));
        if (x) {
            SBTV_HIP(ctx, hipMemcpyAsync(x_out, x, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
            SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        if (numA_out) *numA_out = numA;
        if (numAt_out) *numAt_out = numAt;
        if (n_outer_out) *n_outer_out = last;
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
int csalsa_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, double mu1, double mu2,
               double sigma, double epsilon, double delta, const sbtv_salsa_opts *opts, const double *td,
               const double *xi, double *x_out_dev, double *objective, double *distance1, double *distance2,
               double *criterion, double *times, double *mses, int *numA, int *numAt, int *n_outer, bool spec_wanted) {
    BlurOp c;
    bool spectral = false;
    {
        FftPlan chk;
        SBTV_TRY(fft_plan(ctx, M, N, 1, &chk));
        // spectral form of the constraint split (see `enqueue_spectral` below): needs fixed mu1 / mu2, an even M (pairs of
        // one column per lane) and the row kernels that carry OP_CSALSA
        const bool sp = delta == 1.0 && csalsa_spectral_wanted() && fft_rows_csalsa_ok(chk) && !(M & 1) &&
                        (size_t)M * N < ((size_t)1 << 31);
        SBTV_TRY(admm_common(ctx, M, N, taps, taille, sp ? yd : nullptr, &c));
        spectral = sp;
    }
    const int K = opts->TViters;
    AdmmProx prox;
    SBTV_TRY(prox.plan(ctx, M, N, 1, "prox", K, opts));
    const size_t P = c.P;
    const int nb = ad_blocks(P);
    double *xbuf[2], *u, *bu, *v, *bv, *w, *Ax, *g, *par, *partials, *sums, *acc;
    double2 *Ws;
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * fft_rows_blocks(c.fp), &acc));
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &u));
    SBTV_TRY(ws_get_t(ctx, "admm.bu", P, &bu));
    SBTV_TRY(ws_get_t(ctx, "admm.v", P, &v));
    SBTV_TRY(ws_get_t(ctx, "admm.bv", P, &bv));
    SBTV_TRY(ws_get_t(ctx, "admm.w", P, &w));
    SBTV_TRY(ws_get_t(ctx, "admm.Ax", P, &Ax));
    SBTV_TRY(ws_get_t(ctx, "admm.g", P, &g));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu1, mu2, 1/mu1
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)8 * nb, &partials));
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)64, &sums));            // [0..5] update sums, [6] TV(x), [8] n_ve^2, [16..] prox step sums
    SBTV_TRY(ws_get_t(ctx, "admm.W", c.fp.u_img, &Ws));
    double2 *Es = Ws;                                                   // spectral form: the state spectrum E (W is not formed)
    double *cst = nullptr, *rs = nullptr;
    SBTV_TRY(ws_get_t(ctx, "admm.cs", (size_t)8, &cst));
    SBTV_TRY(ws_get_t(ctx, "admm.rs", (size_t)4, &rs));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    const double *hs = nullptr;
    const int maxiter = opts->maxiter;
    if (!(epsilon != 0.0)) epsilon = sqrt((double)P + 8 * sqrt((double)P)) * sigma;              // :413
    SBTV_TRY(upload_par(ctx, par, {mu1, mu2, 1.0 / mu1, 0.0}));
    run.numAt = 1;                                                       // ATy (:301)
    ctx->calls += 2;                                                     // AT(y), invLS(ATy, mu1) (:301,310)
    double *x = xbuf[0];
    SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, x));
    if (opts->initialization == 0) ctx->calls += 1;
    if (opts->initialization == 2) run.numAt += 1;                       // :385
    SBTV_HIP(ctx, hipMemsetAsync(u, 0, sizeof(double) * P, ctx->stream));   // :404-408
    SBTV_HIP(ctx, hipMemsetAsync(bu, 0, sizeof(double) * P, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(v, 0, sizeof(double) * P, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(bv, 0, sizeof(double) * P, ctx->stream));
    prox.lam = par + 2;                                                  // 1 / mu1
    SBTV_TRY(prox_zero_duals(ctx, prox.pp));                             // :440-441
    SBTV_TRY(prox.arm(ctx, true));

    // state before the loop (:416-448): Ax, criterion(1), objective(1) = TV(x), mses(1), distances
    SBTV_TRY(op_apply(ctx, c, OP_MUL_H, x, Ax));
    run.numA += 2;                                                       // :421,445
    ctx->calls += 2;
    {
        // v = 0, bv = 0, u = 0: the update kernel on scratch multipliers gives the three norms without side effects
        double *sv, *sbv, *sbu;
        SBTV_TRY(ws_get_t(ctx, "admm.scratch0", P, &sv));
        SBTV_TRY(ws_get_t(ctx, "admm.scratch1", P, &sbv));
        SBTV_TRY(ws_get_t(ctx, "admm.scratch2", P, &sbu));
        SBTV_HIP(ctx, hipMemsetAsync(sbv, 0, sizeof(double) * P, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(sbu, 0, sizeof(double) * P, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));   // n_ve^2 = 0 -> inside the ball, v = ve
        hipLaunchKernelGGL(csalsa_update_kernel, dim3(nb), dim3(AB), 0, ctx->stream, Ax, yd, x, u, sv, sbv, sbu, td,
                           (const double *)nullptr, sums + 8, 1.0, partials, P);
        SBTV_TRY(reduce_partials(ctx, partials, 6, nb, sums));
        SBTV_TRY(tvnorm_dev(ctx, x, M, N, 1, sums + 6));
        SBTV_TRY(run.fetch(sums, 8, &hs));
        // before the loop v = 0, so distance1(1) = ||Ax-y-v|| = ||Ax-y|| (:447); hs[1] is not that (v=ve there)
        if (criterion) criterion[0] = sqrt(hs[0]);
        if (distance1) distance1[0] = sqrt(hs[0]);
        if (distance2) distance2[0] = sqrt(hs[2]);                       // ||x - u||, u = 0 (:448)
        if (objective) objective[0] = hs[6];                             // phi(x) = TVnorm(x) (:423)
        if (mses && td) mses[0] = hs[3] / (double)P;                     // :436
        if (times) times[0] = 0.0;
    }
    double crit_prev = sqrt(hs[0]), obj_prev = hs[6];
    SBTV_TRY(run.start());
    // optimistic prox launches need a fixed threshold (the control block is armed once) and the tile kernels
    const bool spec = spec_wanted && delta == 1.0 && prox_spec_ok(prox.pp, g, u, K);
    const int lag = (spec && (opts->speculate & 1)) ? 1 : 0;
    // end of an enqueue: the sums (with the step sums of an optimistic prox) or the iteration count of an exact prox
    auto publish = [&](int outer) {
        return run.publish(outer, sums, 16 + (spec ? K : 0), spec ? K : 0, spec ? nullptr : prox.pp.ctrl);
    };
    const bool tv_fused = fft_cols_tv_ok(c.fp);
    const int ntv = tv_fused ? fft_cols_blocks(c.fp) : 0;
    double *tvp = nullptr;
    if (tv_fused) SBTV_TRY(ws_get_t(ctx, "admm.tvc", (size_t)ntv, &tvp));
    if (spectral) {
        // v = bv = 0 before the loop: E = 0, s_prev = 1
        const double h[8] = {mu2, mu2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        SBTV_HIP(ctx, hipMemsetAsync(Es, 0, sizeof(double2) * c.fp.u_img, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(cst, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    // Spectral form of an outer iteration.  The projection on the epsilon ball scales ve = Ax - y - bv by ONE scalar
    // s = min(1, eps/||ve||) (:485-489), so v = s ve, bv' = bv - (Ax - y - v) = -(1 - s) ve, and the next right-hand side
    // y + v + bv' = y + (2s - 1) ve: the split (v, bv) is the spectrum E of ve and the scalar s.  One row pass then does
    // what took three transforms: W = mu2 (Y + (2 s_prev - 1) E), X = (conj(H) W + mu1 S)/(|H|^2 + mu1), T = H X - Y
    // (= fft2(Ax - y)), E' = T + (1 - s_prev) E, with ||Ax-y||^2, ||ve||^2 and ||E' - E||^2 by Parseval (the norms the
    // traces and the next s need).  Image-domain work left: u + bu into the forward pass, x - bu for the prox, and one
    // pass for bu, TV(x) and the sums over x.
    auto enqueue_spectral = [&](int outer) -> int {
        const int k = outer - 1;
        double *xn = xbuf[k & 1];
        const double *xprev = xbuf[(k & 1) ^ 1];
        RowsArgs a{};
        a.dir_fwd = 1;
        a.dir_inv = 1;
        a.op = OP_CSALSA;
        a.H = c.Hs;
        a.Y = c.Ys;
        a.E = Es;
        a.cs = cst;
        a.mu = par;                                                      // mu1
        a.acc = acc;
        SBTV_TRY(fft_cols_fwd(ctx, c.fp, u, bu, c.S));
        SBTV_TRY(fft_rows(ctx, c.fp, c.S, c.S, a));
        if (fft_cols_inv_step_ok(c.fp)) {
            SBTV_TRY(fft_cols_inv_sub(ctx, c.fp, c.S, xn, c.inv_scale, bu, g));       // x and the prox input x - bu
        } else {
            SBTV_TRY(fft_cols_inv(ctx, c.fp, c.S, xn, c.inv_scale));
            hipLaunchKernelGGL(ad_sub_kernel, dim3(nb), dim3(AB), 0, ctx->stream, xn, bu, g, P);
        }
        hipLaunchKernelGGL(csalsa_scal_kernel, dim3(1), dim3(256), 0, ctx->stream, acc, fft_rows_blocks(c.fp), cst, epsilon,
                           c.parseval, sums);
        RedJobs jb;
        SBTV_TRY(prox.run(ctx, g, u, spec, sums + 16, &jb));             // step sums: reduced with the sums of the last pass
        hipLaunchKernelGGL(csalsa_post_kernel, dim3(nb), dim3(AB), 0, ctx->stream, xn, u, bu, td,
                           (opts->stopcriterion == 2) ? xprev : (const double *)nullptr, partials, (unsigned)M, (unsigned)N, P);
        jb.add(partials, 5, nb, sums + 2);
        SBTV_TRY(reduce_jobs(ctx, jb));
        return publish(outer);
    };
    auto enqueue = [&](int outer) -> int {                               // :461
        if (spectral) return enqueue_spectral(outer);
        const int k = outer - 1;
        double *xn = xbuf[k & 1];
        const double *xprev = xbuf[(k & 1) ^ 1];
        // r = mu1 (u+bu) + mu2 AT(y+v+bv) ; x = invLS(r, mu1)   (:467-471), all in one spectral pass:
        //   X = (conj(H) W + mu1 S) / (|H|^2 + mu1),  W = fft2(mu2 (y+v+bv)),  S = fft2(u+bu)
        hipLaunchKernelGGL(csalsa_w_kernel, dim3(nb), dim3(AB), 0, ctx->stream, yd, v, bv, par, w, P);
        SBTV_TRY(op_spectrum(ctx, c.fp, w, nullptr, c.S, Ws));
        SBTV_TRY(op_solve(ctx, c, u, bu, Ws, par, acc, xn));           // mu1; the residual sum in acc is not used here
        // u = prox_{TV/mu1}(x - bu), warm-started duals (:476)
        hipLaunchKernelGGL(ad_sub_kernel, dim3(nb), dim3(AB), 0, ctx->stream, xn, bu, g, P);
        SBTV_TRY(prox.run(ctx, g, u, spec, sums + 16, nullptr));
        // Ax (the forward column pass of x also leaves the periodic-TV partials of phi(x) = TVnorm(x), :498), projection on
        // the epsilon ball, multipliers, traces (:481-501)
        {
            RowsArgs a{};
            a.dir_fwd = 1;
            a.dir_inv = 1;
            a.op = OP_MUL_H;
            a.H = c.Hs;
            SBTV_TRY(fft_cols_fwd_f(ctx, c.fp, xn, nullptr, c.S, nullptr, tvp));
            SBTV_TRY(fft_rows(ctx, c.fp, c.S, c.S, a));
            SBTV_TRY(fft_cols_inv(ctx, c.fp, c.S, Ax, c.inv_scale));
        }
        hipLaunchKernelGGL(csalsa_ve_kernel, dim3(nb), dim3(AB), 0, ctx->stream, Ax, yd, bv, partials, P);
        SBTV_TRY(reduce_partials(ctx, partials, 1, nb, sums + 8));
        hipLaunchKernelGGL(csalsa_update_kernel, dim3(nb), dim3(AB), 0, ctx->stream, Ax, yd, xn, u, v, bv, bu, td,
                           (opts->stopcriterion == 2) ? xprev : (const double *)nullptr, sums + 8, epsilon, partials, P);
        SBTV_TRY(reduce_partials(ctx, partials, 6, nb, sums));
        if (tv_fused) SBTV_TRY(reduce_partials(ctx, tvp, 1, ntv, sums + 6));
        else SBTV_TRY(tvnorm_dev(ctx, xn, M, N, 1, sums + 6));
        return publish(outer);
    };
    bool stop = false;
    // host side of iteration `outer`: traces (:494-501) and the stop rule (:517-541)
    auto process = [&](int outer) -> int {
        const int k = outer - 1;                                         // the traces start at the first iteration
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        if (spec) SBTV_TRY(prox.check(ctx, hsl + 16));
        run.numAt += 1;
        run.numA += 1;
        ctx->calls += 3;                                                 // AT, invLS, A
        const double crit = sqrt(hsl[0]), obj = hsl[6];
        if (criterion) criterion[k] = crit;                              // :494
        if (distance1) distance1[k] = sqrt(hsl[1]);                      // :495
        if (distance2) distance2[k] = sqrt(hsl[2]);                      // :497
        if (objective) objective[k] = obj;                               // :498
        if (mses && td) mses[k] = hsl[3] / (double)P;                    // :501
        if (times) times[k] = run.seconds();
        if (delta != 1.0) {                                              // :517-518
            mu1 *= delta;
            mu2 *= delta;
            SBTV_TRY(upload_par(ctx, par, {mu1, mu2, 1.0 / mu1, 0.0}));
        }
        double sc;
        if (opts->stopcriterion == 1)
            sc = fabs(obj - obj_prev) / obj;                             // :527
        else if (opts->stopcriterion == 2)
            sc = fabs(sqrt(hsl[4]) / sqrt(hsl[5]));                      // :534
        else
            sc = fabs(crit - crit_prev) / crit;                          // :539
        obj_prev = obj;
        crit_prev = crit;
        stop = (sc < opts->tolA && crit <= epsilon);                     // :529,535,541
        return 0;
    };
    int last = 1;                                                        // the state before the loop is iteration 1 (:416-448)
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[(last - 1) & 1], x_out_dev);
}

// ------------------------------------------------------------------------------------------------
int coral_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, double tau1, double tau2,
              double mu1, double mu2, double mu_ls, int TViters2, const sbtv_salsa_opts *opts, const double *td,
              const double *xi, double *x_out_dev, double *objective, double *distance, double *times, double *mses,
              int *numA, int *numAt, int *n_outer, bool spec_wanted) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, yd, &c));
    // The two TV proxes of an iteration are independent (:401,406).  With the same iteration count they run as ONE batch of
    // two images (own threshold, own duals, own stop rule per image: the batch semantics of the prox): two Chambolle
    // launches with twice the tiles per outer iteration instead of four (SBTV_CORAL_BATCH=0: one plan per prox)
    static const bool env_batch = [] {
        const char *e = getenv("SBTV_CORAL_BATCH");
        return !(e && e[0] == '0');
    }();
    const bool batched = env_batch && opts->TViters == TViters2;
    const int K1 = opts->TViters, K2 = TViters2;
    AdmmProx pu, pv;                                                     // batched: pu is the plan of both images
    SBTV_TRY(pu.plan(ctx, M, N, batched ? 2 : 1, batched ? "prox.pair" : "prox", K1, opts));
    if (!batched) SBTV_TRY(pv.plan(ctx, M, N, 1, "prox2", K2, opts));
    const size_t P = c.P;
    const int nb = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    const bool tv_in_s = !(M & 1) && P < ((size_t)1 << 31);             // TV(u), TV(v) ride in the pass that forms s
    double *xbuf[2], *u, *bu, *v, *bv, *s, *g1, *g2, *par, *partials, *sums, *acc, *tvpart;
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.uv", 2 * P, &u));                      // [u | v] and [g1 | g2]: the images of the batch
    v = u + P;
    SBTV_TRY(ws_get_t(ctx, "admm.bu", P, &bu));
    SBTV_TRY(ws_get_t(ctx, "admm.bv", P, &bv));
    SBTV_TRY(ws_get_t(ctx, "admm.w", P, &s));
    SBTV_TRY(ws_get_t(ctx, "admm.g12", 2 * P, &g1));
    g2 = g1 + P;
    SBTV_TRY(ws_get_t(ctx, "admm.tvpart", (size_t)2 * nb, &tvpart));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu_ls, thr1, thr2
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)8 * nb, &partials));
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));            // [0..6] post sums, [8] resid2, [9] TV(u), [10] TV(v), [16..], [48..] step sums
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    SBTV_TRY(upload_par(ctx, par, {mu_ls, tau1 / mu1, tau2 / mu2, 0.0}));   // thresholds :356,361
    pu.lam = par + 1;
    pv.lam = par + 2;
    const int maxiter = opts->maxiter;
    run.numAt = 2;                                                       // ATy twice (:189,219)
    ctx->calls += 3;                                                     // AT(y), invLS(ATy), AT(y)
    double *x = xbuf[0];
    SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, x));
    if (opts->initialization == 0) ctx->calls += 1;
    // u = x ; bu = u ; v = x ; bv = v  (:353-359)  ->  first prox inputs x - bu = x - bv = 0
    for (double *dst : {u, bu, v, bv})
        SBTV_HIP(ctx, hipMemcpyAsync(dst, x, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(g1, 0, sizeof(double) * P, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(g2, 0, sizeof(double) * P, ctx->stream));
    SBTV_TRY(prox_zero_duals(ctx, pu.pp));                               // :384-392
    SBTV_TRY(pu.arm(ctx, true));
    if (!batched) {
        SBTV_TRY(prox_zero_duals(ctx, pv.pp));
        SBTV_TRY(pv.arm(ctx, true));
    }

    // initial objective (:366-368)
    double obj_prev;
    {
        SBTV_TRY(op_resid(ctx, c, x, acc));
        SBTV_TRY(reduce_partials(ctx, acc, 1, nrb, sums + 8));
        SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 9));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 8, ctx->stream));
        if (td) {
            double *o4 = nullptr;
            SBTV_TRY(ws_get_t(ctx, "admm.o4", (size_t)4, &o4));
            SBTV_TRY(pair_sums(ctx, x, td, P, 1, o4));
            SBTV_HIP(ctx, hipMemcpyAsync(sums, o4, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        }
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        run.numA += 1;
        ctx->calls += 1;
        obj_prev = 0.5 * (hs[8] * c.parseval) + tau1 * hs[9] + tau2 * hs[9];   // u = v = x
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[0] / (double)P;                     // :381
    }
    SBTV_TRY(run.start());
    const bool spec = spec_wanted && prox_spec_ok(pu.pp, g1, u, K1) &&
                      (batched || prox_spec_ok(pv.pp, g2, v, K2));
    const int lag = (spec && (opts->speculate & 1)) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {                               // :394
        double *xn = xbuf[outer & 1];
        const double *xprev = xbuf[(outer & 1) ^ 1];
        // the two TV proxes with their own warm-started duals (:401,406).  The first outer iteration always runs exactly:
        // its prox inputs x - bu = x - bv are zero and the rule stops at k = 1; its control blocks are re-armed afterwards
        const bool sp = spec && outer >= 2;
        RedJobs jb;
        if (spec && outer == 2) {
            SBTV_TRY(pu.arm(ctx, false));
            if (!batched) SBTV_TRY(pv.arm(ctx, false));
        }
        if (batched) {
            // both images in one plan: the step sums of image b land at sums + 16 + b FSTRIDE (= sums + 48 for v), reduced
            // at the end of the iteration
            static_assert(FSTRIDE == 32, "the step sums of the second prox are read at sums + 48");
            SBTV_TRY(pu.run(ctx, g1, u, sp, sums + 16, &jb));
        } else {
            SBTV_TRY(pu.run(ctx, g1, u, sp, sums + 16, nullptr));
            SBTV_TRY(pv.run(ctx, g2, v, sp, sums + 48, nullptr));
        }
        // r = ATy + mu1 (u+bu) + mu2 (v+bv) ; x = invLS(r)   (:411-413)  + residual energy (:423, Parseval)
        if (tv_in_s) {
            hipLaunchKernelGGL(coral_s_kernel<true>, dim3(nb), dim3(AB), 0, ctx->stream, u, bu, v, bv, mu1, mu2, mu_ls, s, tvpart,
                               (unsigned)M, (unsigned)N, P);
            jb.add(tvpart, 2, nb, sums + 9);
        } else {
            hipLaunchKernelGGL(coral_s_kernel<false>, dim3(nb), dim3(AB), 0, ctx->stream, u, bu, v, bv, mu1, mu2, mu_ls, s, tvpart,
                               (unsigned)M, (unsigned)N, P);
        }
        SBTV_TRY(op_solve(ctx, c, s, nullptr, c.Ys, par, acc, xn));    // mu_ls
        hipLaunchKernelGGL(coral_post_kernel, dim3(nb), dim3(AB), 0, ctx->stream, xn,
                           (opts->stopcriterion == 2) ? xprev : (const double *)nullptr, u, v, bu, bv, g1, g2, td, partials, P);
        jb.add(partials, 7, nb, sums);
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        if (!tv_in_s) {
            SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 9));
            SBTV_TRY(tvnorm_dev(ctx, v, M, N, 1, sums + 10));
        }
        if (sp) return run.publish(outer, sums, 80, K1 + K2);
        return run.publish(outer, sums, 12, 0, pu.pp.ctrl, batched ? pu.pp.ctrl + 1 : pv.pp.ctrl);
    };
    bool stop = false;
    auto process = [&](int outer) -> int {
        const double *hsl;
        const bool sp = spec && outer >= 2;
        SBTV_TRY(run.wait(outer, &hsl));
        if (sp) {     // per plan: batched, the step sums of v are those of the plan's second image (sums + 48)
            SBTV_TRY(pu.check(ctx, hsl + 16));
            if (!batched) SBTV_TRY(pv.check(ctx, hsl + 48));
        }
        run.numA += 1;
        ctx->calls += 2;                                                 // invLS, A
        const double f = 0.5 * (hsl[8] * c.parseval) + tau1 * hsl[9] + tau2 * hsl[10];      // :425
        if (objective) objective[outer] = f;
        if (mses && td) mses[outer] = hsl[0] / (double)P;                // :428-429
        if (distance) {
            distance[(size_t)(outer - 1) * 2] = sqrt(hsl[1]) / sqrt(hsl[3] + hsl[4]);       // :432
            distance[(size_t)(outer - 1) * 2 + 1] = sqrt(hsl[2]) / sqrt(hsl[3] + hsl[5]);   // :433
        }
        if (times) times[outer] = run.seconds();
        stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[6], hsl[3], opts->tolA);
        obj_prev = f;
        return 0;
    };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[last & 1], x_out_dev);
}

// ------------------------------------------------------------------------------------------------
// Masked-observation SALSA:  min_x 0.5 sum(m .* (B x - y).^2) + tau TV(x)  with the splits u = x (TV) and v = B x (data),
// the ADMM of Almeida & Figueiredo (IEEE TIP 2013) in SALSA_v2's sign convention (include/sbtv.h states the iteration).
// The spectral solve with its two right-hand sides,
//     X = (mu1 fft2(u+bu) + mu2 conj(H) fft2(v+bv)) / (mu1 + mu2 |H|^2)
//       = (conj(H) W + r S) / (|H|^2 + r),   W = fft2(v+bv), S = fft2(u+bu), r = mu1 / mu2,
// is the row pass OP_SALSA with the per-iteration spectrum W in the place of fft2(y) and r in the place of mu: no new
// row kernel.  Bx needs no forward column pass either: the row pass leaves S = N colFFT(x) (the column-transformed x), so a
// second row pass with OP_MUL_H on that S and an inverse column pass scaled by 1/N more give real(ifft2(H X)).  Per outer
// iteration: 2 forward column passes (v+bv, u+bu), 3 row passes (+ the unpack of W), 2 inverse column passes, the prox,
// one element-wise pass and one reduction launch.
int masked_one(sbtv_ctx *ctx, const double *yd, const double *md, int M, int N, const double *taps, int taille, double tau,
               double mu1, double mu2, const sbtv_salsa_opts *opts, const double *td, const double *xi, double *x_out_dev,
               double *objective, double *distance, double *times, double *mses, int *numA, int *numAt, int *n_outer,
               bool spec_wanted) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, nullptr, &c));
    const int K = opts->TViters;
    AdmmProx prox;
    SBTV_TRY(prox.plan(ctx, M, N, 1, "prox", K, opts));
    const size_t P = c.P;
    const int nb = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    const bool tv_in_post = !(M & 1) && P < ((size_t)1 << 31);          // TV(u) rides in the element-wise pass
    const int nq = tv_in_post ? 10 : 9;
    double *xbuf[2], *u, *bu, *v, *bv, *Bx, *g, *par, *partials, *sums, *acc;
    double2 *Ws, *S2;
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &u));
    SBTV_TRY(ws_get_t(ctx, "admm.bu", P, &bu));
    SBTV_TRY(ws_get_t(ctx, "admm.v", P, &v));
    SBTV_TRY(ws_get_t(ctx, "admm.bv", P, &bv));
    SBTV_TRY(ws_get_t(ctx, "admm.Ax", P, &Bx));
    SBTV_TRY(ws_get_t(ctx, "admm.g", P, &g));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu1 / mu2, tau / mu1
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * nb, &partials));
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));            // [0..9] sums of the element-wise pass, [16..] prox step sums
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));         // residual sum of OP_SALSA (against W: not used)
    SBTV_TRY(ws_get_t(ctx, "admm.W", c.fp.u_img, &Ws));
    SBTV_TRY(ws_get_t(ctx, "admm.S2", c.fp.s_img, &S2));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    SBTV_TRY(upload_par(ctx, par, {mu1 / mu2, tau / mu1, 0.0, 0.0}));
    prox.lam = par + 1;
    // the inverse column pass of H X takes the spectrum the row pass of X left: N times the column transform of x (the
    // chirp-z path keeps whole 2-D spectra, its "row pass" is point-wise)
    const double bx_scale = c.fp.generic ? c.inv_scale : c.inv_scale / (double)N;
    auto post = [&](const double *xn, const double *xprev) {
        if (tv_in_post)
            hipLaunchKernelGGL(masked_post_kernel<true>, dim3(nb), dim3(AB), 0, ctx->stream, xn, xprev, (const double *)Bx,
                               (const double *)u, yd, md, bu, v, bv, g, td, mu2, partials, (unsigned)M, (unsigned)N, P);
        else
            hipLaunchKernelGGL(masked_post_kernel<false>, dim3(nb), dim3(AB), 0, ctx->stream, xn, xprev, (const double *)Bx,
                               (const double *)u, yd, md, bu, v, bv, g, td, mu2, partials, (unsigned)M, (unsigned)N, P);
    };
    const int maxiter = opts->maxiter;
    double *x = xbuf[0];
    if (opts->initialization == 2) {                                     // x = B'(m .* y)
        hipLaunchKernelGGL(masked_my_kernel, dim3(nb), dim3(AB), 0, ctx->stream, md, yd, g, P);
        SBTV_TRY(op_apply(ctx, c, OP_MUL_HC, g, x));
        run.numAt += 1;
        ctx->calls += 1;
    } else {
        SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, x));
    }
    // Bx = B x ; u = x ; v = Bx ; bu = bv = 0 ; zero duals.  The element-wise pass on that state leaves bu = bv = 0, the
    // first prox input g = x, the first v and the sums of objective(1) / mses(1)
    SBTV_TRY(op_apply(ctx, c, OP_MUL_H, x, Bx));
    run.numA += 1;
    ctx->calls += 1;
    SBTV_HIP(ctx, hipMemcpyAsync(u, x, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemcpyAsync(v, Bx, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(bu, 0, sizeof(double) * P, ctx->stream));
    SBTV_HIP(ctx, hipMemsetAsync(bv, 0, sizeof(double) * P, ctx->stream));
    SBTV_TRY(prox_zero_duals(ctx, prox.pp));
    SBTV_TRY(prox.arm(ctx, true));
    double obj_prev;
    {
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));
        post(x, nullptr);
        SBTV_TRY(reduce_partials(ctx, partials, nq, nb, sums));
        if (!tv_in_post) SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 9));
        SBTV_HIP(ctx, hipGetLastError());
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        obj_prev = 0.5 * hs[0] + tau * hs[9];
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[7] / (double)P;
    }
    SBTV_TRY(run.start());
    const bool spec = spec_wanted && prox_spec_ok(prox.pp, g, u, K);
    const int lag = (spec && (opts->speculate & 1)) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {
        double *xn = xbuf[outer & 1];
        const double *xprev = xbuf[(outer & 1) ^ 1];
        // u = prox_{(tau/mu1) TV}(x - bu), warm-started duals.  The first outer iteration always runs exactly (a zero start
        // gives a zero prox input and the rule stops at k = 1); the control block is re-armed for the optimistic launches
        const bool sp = spec && outer >= 2;
        RedJobs jb;
        if (spec && outer == 2) SBTV_TRY(prox.arm(ctx, false));
        SBTV_TRY(prox.run(ctx, g, u, sp, sums + 16, &jb));               // step sums: reduced at the end of the iteration
        // W = fft2(v + bv) (v was formed by the previous element-wise pass)
        SBTV_TRY(op_spectrum(ctx, c.fp, v, bv, S2, Ws));
        // X = (conj(H) W + r fft2(u + bu)) / (|H|^2 + r), r = mu1 / mu2 ; x = real(ifft2(X))
        SBTV_TRY(op_solve(ctx, c, u, bu, Ws, par, acc, xn));
        // Bx = real(ifft2(H X)) from the column-transformed x the row pass left in S
        {
            RowsArgs a{};
            a.dir_fwd = 1;
            a.dir_inv = 1;
            a.op = OP_MUL_H;
            a.H = c.Hs;
            SBTV_TRY(fft_rows(ctx, c.fp, c.S, S2, a));
            SBTV_TRY(fft_cols_inv(ctx, c.fp, S2, Bx, bx_scale));
        }
        post(xn, (opts->stopcriterion == 2) ? xprev : (const double *)nullptr);
        jb.add(partials, nq, nb, sums);
        SBTV_TRY(reduce_jobs(ctx, jb));
        if (!tv_in_post) SBTV_TRY(tvnorm_dev(ctx, u, M, N, 1, sums + 9));
        return run.publish(outer, sums, sp ? 16 + K : 12, sp ? K : 0, sp ? nullptr : prox.pp.ctrl);
    };
    bool stop = false;
    // host side of iteration `outer`: traces and the stop rule of SALSA_v2.m:442-482
    auto process = [&](int outer) -> int {
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        if (spec && outer >= 2) SBTV_TRY(prox.check(ctx, hsl + 16));
        run.numA += 1;                                                   // H .* X
        run.numAt += 1;                                                  // conj(H) .* fft2(v + bv)
        ctx->calls += 2;
        const double f = 0.5 * hsl[0] + tau * hsl[9];
        if (objective) objective[outer] = f;
        if (mses && td) mses[outer] = hsl[7] / (double)P;
        if (distance) {
            distance[(size_t)(outer - 1) * 2] = sqrt(hsl[1]) / sqrt(hsl[3] + hsl[4]);
            distance[(size_t)(outer - 1) * 2 + 1] = sqrt(hsl[2]) / sqrt(hsl[5] + hsl[6]);
        }
        if (times) times[outer] = run.seconds();
        stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[8], hsl[3], opts->tolA);
        obj_prev = f;
        return 0;
    };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[last & 1], x_out_dev);
}

// ------------------------------------------------------------------------------------------------
// Wavelet-l1 deconvolution in the synthesis form (SALSA/run_deblur_synthesis_L1.m:160-180):
//     min over xw   0.5 ||y - B W xw||^2 + tau ||xw||_1,
// W the Parseval frame of wavelet.hip (W W' = I), solved as SALSA_v2.m:389-494 does with Psi = soft, Phi = l1, A = B W,
// AT = W' B' and invLS(r) = (r - W' F W r) / mu, F = |H|^2 / (|H|^2 + mu) in the Fourier domain.  With W W' = I one outer
// iteration of that is exactly
//     u = soft(xw - bu, tau / mu) ; s = u + bu ; z = W s ;
//     X = (conj(H) fft2(y) + mu fft2(z)) / (|H|^2 + mu) ; xi = real(ifft2(X))      (the row pass OP_SALSA on z)
//     we = W'(xi - z) ; xw = s + we ; bu = -we
// with the image estimate W xw = xi and ||y - B xi||^2 from the row pass's Parseval sum.  The coefficient state is (s, we):
// the next prox input is s + 2 we.  Both and xi are double-buffered, so the result of the stopping iteration is intact when
// the host evaluates the stop rule one iteration late.  Per outer iteration: the prox pass, one synthesis (J launches), the
// FFT triple, the difference, one analysis (J launches), the sums pass and one reduction launch.
int wavelet_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, const WavPlan &wp, double tau,
                double mu, const sbtv_salsa_opts *opts, const double *td, const double *xwi, double *xw_out_dev,
                double *x_out_dev, double *objective, double *distance, double *times, double *mses, int *numA, int *numAt,
                int *n_outer) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, yd, &c));
    const size_t P = c.P, C = P * wp.bands();
    const int nb = ad_blocks(C), nbp = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    double *sbuf[2], *wbuf[2], *xibuf[2], *z, *d, *par, *partials, *sums, *acc;
    SBTV_TRY(ws_get_t(ctx, "wav.s0", C, &sbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.s1", C, &sbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "wav.we0", C, &wbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.we1", C, &wbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xibuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xibuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &z));
    SBTV_TRY(ws_get_t(ctx, "admm.g", P, &d));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * 1024, &partials));   // [0..1] prox sums, [2..5] post sums, nb each
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));            // [0] |u|, [1] u^2, [2..5] post sums, [8] resid2
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    SBTV_TRY(upload_par(ctx, par, {mu, 0.0, 0.0, 0.0}));
    const double T = tau / mu;                                           // :394
    const int maxiter = opts->maxiter;
    run.numAt = 1;                                                       // ATy (:288)
    ctx->calls += 2;                                                     // AT(y), invLS(ATy)
    // the start xw as the state (s, we) = (xw, 0): bu = -we = 0 (:367-393)
    double *s0 = sbuf[0];
    if (opts->initialization == 0) {
        SBTV_HIP(ctx, hipMemsetAsync(s0, 0, sizeof(double) * C, ctx->stream));
        ctx->calls += 1;
    } else if (opts->initialization == 2) {                              // xw = W' B' y
        SBTV_TRY(op_apply(ctx, c, OP_MUL_HC, yd, d));
        SBTV_TRY(wav_analysis(ctx, wp, d, s0, 1));
    } else {
        SBTV_HIP(ctx, hipMemcpyAsync(s0, xwi, sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
    }
    SBTV_HIP(ctx, hipMemsetAsync(wbuf[0], 0, sizeof(double) * C, ctx->stream));
    // initial objective (:399-401): resid = y - B W xw
    double obj_prev;
    {
        SBTV_TRY(wav_synthesis(ctx, wp, s0, xibuf[0], 1));
        SBTV_TRY(op_resid(ctx, c, xibuf[0], acc));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));
        hipLaunchKernelGGL(wav_init_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)s0, td, partials, C);
        RedJobs jb;
        jb.add(partials, 2, nb, sums);
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        SBTV_HIP(ctx, hipGetLastError());
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        run.numA += 1;
        ctx->calls += 1;
        obj_prev = 0.5 * (hs[8] * c.parseval) + tau * hs[0];
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[1] / (double)C;                     // :414
    }
    SBTV_TRY(run.start());
    const int lag = (opts->speculate & 1) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {                               // :423
        const int o = outer & 1, p = o ^ 1;
        double *sn = sbuf[o], *wn = wbuf[o], *xi = xibuf[o];
        const double *sp = sbuf[p], *we = wbuf[p];
        hipLaunchKernelGGL(wav_prox_kernel, dim3(nb), dim3(AB), 0, ctx->stream, sp, we, sn, T, partials, C);      // :432
        SBTV_TRY(wav_synthesis(ctx, wp, sn, z, 1));
        SBTV_TRY(op_solve(ctx, c, z, nullptr, c.Ys, par, acc, xi));    // :434-436
        hipLaunchKernelGGL(ad_sub_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)xi, (const double *)z, d, P);
        SBTV_TRY(wav_analysis(ctx, wp, d, wn, 1));
        hipLaunchKernelGGL(wav_post_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)sn, (const double *)wn, we,
                           (opts->stopcriterion == 2) ? sp : (const double *)nullptr, td, partials + (size_t)2 * nb, C);
        RedJobs jb;
        jb.add(partials, 6, nb, sums);
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        return run.publish(outer, sums, 12, 0);
    };
    bool stop = false;
    // host side of iteration `outer`: traces and the stop rule of SALSA_v2.m:442-482
    auto process = [&](int outer) -> int {
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        run.numA += 1;                                                   // :443
        ctx->calls += 2;                                                 // invLS, A
        const double f = 0.5 * (hsl[8] * c.parseval) + tau * hsl[0];     // :444
        if (objective) objective[outer] = f;
        if (mses && td) mses[outer] = hsl[4] / (double)C;                // :446-449
        if (distance) distance[outer - 1] = sqrt(hsl[2]) / sqrt(hsl[3] + hsl[1]);   // :451
        if (times) times[outer] = run.seconds();
        stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[5], hsl[3], opts->tolA);
        obj_prev = f;
        return 0;
    };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    SBTV_TRY(run.finish(P, last, nullptr, nullptr));                     // the result: xw = s + we, and the image xi
    hipLaunchKernelGGL(wav_sum_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)sbuf[last & 1],
                       (const double *)wbuf[last & 1], xw_out_dev, C);
    SBTV_HIP(ctx, hipGetLastError());
    if (x_out_dev)
        SBTV_HIP(ctx, hipMemcpyAsync(x_out_dev, xibuf[last & 1], sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Wavelet-l1 deconvolution in the analysis form, the 'P' / 'PT' mode of SALSA_v2.m (:98-101, 198-203):
//     min over the image x   0.5 ||y - B x||^2 + tau ||W' x||_1,
// solved as SALSA_v2.m:389-494 does with Psi = soft, Phi = l1, A = B, AT = B', PT = W', P = W and invLS(r) =
// real(ifft2(fft2(r) ./ (|H|^2 + mu))), the exact x-minimiser because W W' = I.  One outer iteration k on the coefficient
// state (s, bu), s = u + bu:
//     z = W s_k ;  X = (conj(H) fft2(y) + mu fft2(z)) / (|H|^2 + mu) ;  x_k = real(ifft2(X))      (the row pass OP_SALSA on z)
//     w_k = W' x_k ;  the step pass (wav_astep_kernel): u_k = s_k - bu_{k-1}, its sums, bu_k, s_{k+1}
// with ||y - B x_k||^2 from the row pass's Parseval sum and the image-domain sums of x_k from a pixel pass, launched only when
// 'TRUE_X' or stop rule 2 ask for them.  s, bu and x are double-buffered, so the result of the stopping iteration is intact
// when the host evaluates the stop rule one iteration late.  Per outer iteration: one synthesis (J launches), the FFT triple,
// one analysis (J launches), the step pass, the pixel pass and one reduction launch.
int analysis_one(sbtv_ctx *ctx, const double *yd, int M, int N, const double *taps, int taille, const WavPlan &wp, double tau,
                 double mu, const sbtv_salsa_opts *opts, const double *td, const double *xi, double *x_out_dev,
                 double *objective, double *distance, double *times, double *mses, int *numA, int *numAt, int *n_outer) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, yd, &c));
    const size_t P = c.P, C = P * wp.bands();
    const int nb = ad_blocks(C), nbp = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    double *sbuf[2], *bbuf[2], *xbuf[2], *w, *z, *par, *partials, *sums, *acc;
    SBTV_TRY(ws_get_t(ctx, "wav.s0", C, &sbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.s1", C, &sbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "wav.we0", C, &bbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.we1", C, &bbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "wav.w", C, &w));
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &xbuf[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &xbuf[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &z));
    SBTV_TRY(ws_get_t(ctx, "admm.par", (size_t)4, &par));               // mu
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * 1024, &partials));   // [0..3] step sums, nb each, then [0..2] pixel sums, nbp each
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));            // [0..3] step sums, [4..6] pixel sums, [8] resid2
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));
    double *ppix = partials + (size_t)4 * nb;
    AdmmRun run;
    SBTV_TRY(run.open(ctx, numA, numAt, n_outer));
    SBTV_TRY(upload_par(ctx, par, {mu, 0.0, 0.0, 0.0}));
    const double T = tau / mu;                                           // :394
    const int maxiter = opts->maxiter;
    const bool rule2 = opts->stopcriterion == 2;
    run.numAt = 1;                                                       // ATy (:288)
    ctx->calls += 2;                                                     // AT(y), invLS(ATy)
    if (opts->initialization == 0) ctx->calls += 1;                      // AT(zeros) (:369)
    SBTV_TRY(op_init_x(ctx, c, opts->initialization, yd, xi, xbuf[0]));  // :367-381
    // PTx = W'x ; u = PTx ; bu = 0 (:389-393) and the initial objective (:399-401): the step pass on (s, bu) = (PTx, 0)
    double obj_prev;
    {
        SBTV_TRY(wav_analysis(ctx, wp, xbuf[0], w, 1));
        SBTV_HIP(ctx, hipMemsetAsync(bbuf[1], 0, sizeof(double) * C, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));
        hipLaunchKernelGGL(wav_astep_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)w, (const double *)bbuf[1],
                           (const double *)w, bbuf[0], sbuf[0], T, partials, C);
        SBTV_TRY(op_resid(ctx, c, xbuf[0], acc));
        RedJobs jb;
        jb.add(partials, 4, nb, sums);
        if (td) {
            hipLaunchKernelGGL(ad_xsums_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)xbuf[0], td,
                               (const double *)nullptr, ppix, P);
            jb.add(ppix, 3, nbp, sums + 4);
        }
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        SBTV_HIP(ctx, hipGetLastError());
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        run.numA += 1;
        ctx->calls += 1;
        obj_prev = 0.5 * (hs[8] * c.parseval) + tau * hs[0];
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[4] / (double)P;                     // :415
    }
    SBTV_TRY(run.start());
    const int lag = (opts->speculate & 1) ? 1 : 0;
    auto enqueue = [&](int outer) -> int {                               // :423
        const int o = outer & 1, p = o ^ 1;
        double *xn = xbuf[o];
        SBTV_TRY(wav_synthesis(ctx, wp, sbuf[p], z, 1));                 // P(u + bu) (:434)
        SBTV_TRY(op_solve(ctx, c, z, nullptr, c.Ys, par, acc, xn));      // :434-436
        SBTV_TRY(wav_analysis(ctx, wp, xn, w, 1));                       // :438
        hipLaunchKernelGGL(wav_astep_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)sbuf[p],
                           (const double *)bbuf[p], (const double *)w, bbuf[o], sbuf[o], T, partials, C);   // :440, :431
        RedJobs jb;
        jb.add(partials, 4, nb, sums);
        if (td || rule2) {
            hipLaunchKernelGGL(ad_xsums_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)xn, td,
                               rule2 ? (const double *)xbuf[p] : (const double *)nullptr, ppix, P);
            jb.add(ppix, 3, nbp, sums + 4);
        }
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        return run.publish(outer, sums, 12, 0);
    };
    bool stop = false;
    // host side of iteration `outer`: traces and the stop rule of SALSA_v2.m:442-482
    auto process = [&](int outer) -> int {
        const double *hsl;
        SBTV_TRY(run.wait(outer, &hsl));
        run.numA += 1;                                                   // :443
        ctx->calls += 2;                                                 // invLS, A
        const double f = 0.5 * (hsl[8] * c.parseval) + tau * hsl[0];     // :444
        if (objective) objective[outer] = f;
        if (mses && td) mses[outer] = hsl[4] / (double)P;                // :446-449
        if (distance) distance[outer - 1] = sqrt(hsl[2]) / sqrt(hsl[3] + hsl[1]);   // :451
        if (times) times[outer] = run.seconds();
        stop = salsa_stop(opts->stopcriterion, outer, f, obj_prev, hsl[5], hsl[6], opts->tolA);
        obj_prev = f;
        return 0;
    };
    int last = 0;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiter, lag, false, enqueue, process, [&] { return !stop; }));
    return run.finish(P, last, xbuf[last & 1], x_out_dev);
}

// ------------------------------------------------------------------------------------------------
// FISTA on the same problem (SALSA/my_fista_l1.m:5-68): min over x  0.5 ||b - B W x||^2 + tau ||x||_1.  The reference's
// iteration k = 2..maxiters is (:34-47)
//     y = y - (1/L) W'B'(B W y - b) ; x = soft(y, tau/L) ; t = 0.5 (1 + sqrt(1 + 4 t_old^2)) ; y = x + ((t_old-1)/t)(x - x_old)
//     objective(k) = 0.5 ||B W x - b||^2 + tau sum|x|
// What runs keeps x_{k-1}, x_{k-2} and their images zx = W x in two buffers each and never stores y: with c the momentum
// factor of the iteration before (0 for k = 2; t and c depend on no data, the host knows them when it enqueues)
//     zy = zx_{k-1} + c (zx_{k-1} - zx_{k-2})              (= W y by linearity; fl1_momentum_kernel)
//     g  = W' B'(B zy - b)                                  (op_gradf, wav_analysis)
//     x_k = soft((x_{k-1} + c (x_{k-1} - x_{k-2})) - (1/L) g, tau/L)   over x_{k-2}, with its sums (fl1_step_kernel)
//     zx_k = W x_k over zx_{k-2} ; ||B zx_k - b||^2         (wav_synthesis, op_resid)
// one synthesis per iteration where the reference has two (W y inside A(y), W x for the objective).  The host books the
// traces and the stop rule one iteration late (lag 1); iteration k + 1 writes the buffers of x_{k-1}, so x_k and zx_k are
// intact when the rule of iteration k is seen.
int fista_l1_one(sbtv_ctx *ctx, const double *bd, int M, int N, const double *taps, int taille, const WavPlan &wp, double tau,
                 double L, int stopcriterion, double tolerance, int maxiters, int lag, const double *td, const double *xwi,
                 double *xw_out_dev, double *x_out_dev, double *objective, double *times, double *mses, int *n_iter) {
    BlurOp c;
    SBTV_TRY(admm_common(ctx, M, N, taps, taille, bd, &c));
    const size_t P = c.P, C = P * wp.bands();
    const int nb = ad_blocks(C), nbp = ad_blocks(P), nrb = fft_rows_blocks(c.fp);
    double *xb[2], *zb[2], *zy, *gi, *g, *partials, *sums, *acc;
    SBTV_TRY(ws_get_t(ctx, "wav.s0", C, &xb[0]));
    SBTV_TRY(ws_get_t(ctx, "wav.s1", C, &xb[1]));
    SBTV_TRY(ws_get_t(ctx, "wav.we0", C, &g));
    SBTV_TRY(ws_get_t(ctx, "admm.x0", P, &zb[0]));
    SBTV_TRY(ws_get_t(ctx, "admm.x1", P, &zb[1]));
    SBTV_TRY(ws_get_t(ctx, "admm.u", P, &zy));
    SBTV_TRY(ws_get_t(ctx, "admm.g", P, &gi));
    SBTV_TRY(ws_get_t(ctx, "admm.partials", (size_t)12 * 1024, &partials));   // [0..3] step sums, nb each
    SBTV_TRY(ws_get_t(ctx, "admm.sums", (size_t)96, &sums));            // [0] |x|, [1] x^2, [2] (x-xprev)^2, [3] (x-true)^2, [8] resid2
    SBTV_TRY(ws_get_t(ctx, "admm.acc", (size_t)3 * nrb, &acc));
    AdmmRun run;
    SBTV_TRY(run.open(ctx, nullptr, nullptr, n_iter));
    const double T = tau / L, invL = 1.0 / L;                            // :38-39
    const int nq = td ? 4 : 3;
    ctx->calls += 2;                                                     // AT(b) (:20), A(x) (:28)
    // iterate 1, the start (:20-22; x = y = xw_init): in the buffers of parity 1, and as "x_0" in those of parity 0, where
    // c = 0 multiplies a zero difference
    if (xwi) {
        SBTV_HIP(ctx, hipMemcpyAsync(xb[1], xwi, sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
        SBTV_HIP(ctx, hipMemcpyAsync(xb[0], xwi, sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        SBTV_HIP(ctx, hipMemsetAsync(xb[1], 0, sizeof(double) * C, ctx->stream));
        SBTV_HIP(ctx, hipMemsetAsync(xb[0], 0, sizeof(double) * C, ctx->stream));
    }
    double obj_prev;
    {
        SBTV_TRY(wav_synthesis(ctx, wp, xb[1], zb[1], 1));               // :27-29
        SBTV_HIP(ctx, hipMemcpyAsync(zb[0], zb[1], sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
        SBTV_TRY(op_resid(ctx, c, zb[1], acc));
        SBTV_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(double) * 16, ctx->stream));
        hipLaunchKernelGGL(wav_init_kernel, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)xb[1], td, partials, C);
        RedJobs jb;
        jb.add(partials, 2, nb, sums);
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        SBTV_HIP(ctx, hipGetLastError());
        const double *hs;
        SBTV_TRY(run.fetch(sums, 16, &hs));
        obj_prev = 0.5 * (hs[8] * c.parseval) + tau * hs[0];
        if (objective) objective[0] = obj_prev;
        if (times) times[0] = 0.0;
        if (mses && td) mses[0] = hs[1] / (double)C;                     // :29
    }
    SBTV_TRY(run.start());
    double t_enq = 1.0, c_enq = 0.0;                                     // t and the momentum factor as the next enqueue sees them
    auto enqueue = [&](int k) -> int {                                   // :34
        const int o = k & 1, p = o ^ 1;
        const double cm = c_enq;
        hipLaunchKernelGGL(fl1_momentum_kernel, dim3(nbp), dim3(AB), 0, ctx->stream, (const double *)zb[p],
                           (const double *)zb[o], cm, zy, P);
        SBTV_TRY(op_gradf(ctx, c, zy, acc, gi));                         // :38; its residual sum (of the momentum point) is not used
        SBTV_TRY(wav_analysis(ctx, wp, gi, g, 1));
        if (td)
            hipLaunchKernelGGL(fl1_step_kernel<true>, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)xb[p], xb[o],
                               (const double *)g, td, cm, invL, T, partials, C);
        else
            hipLaunchKernelGGL(fl1_step_kernel<false>, dim3(nb), dim3(AB), 0, ctx->stream, (const double *)xb[p], xb[o],
                               (const double *)g, td, cm, invL, T, partials, C);
        SBTV_TRY(wav_synthesis(ctx, wp, xb[o], zb[o], 1));               // :43
        SBTV_TRY(op_resid(ctx, c, zb[o], acc));                          // :44
        RedJobs jb;
        jb.add(partials, nq, nb, sums);
        jb.add(acc, 1, nrb, sums + 8);
        SBTV_TRY(reduce_jobs(ctx, jb));
        const double t_old = t_enq;
        t_enq = 0.5 * (1 + sqrt(1 + 4 * t_old * t_old));                 // :41
        c_enq = (t_old - 1) / t_enq;                                     // :42
        return run.publish(k, sums, 12, 0);
    };
    bool stop = false;
    // host side of iteration k: traces and the stop rule (:44-66)
    auto process = [&](int k) -> int {
        const double *hsl;
        SBTV_TRY(run.wait(k, &hsl));
        ctx->calls += 3;                                                 // A(y), AT, A(x)
        const double f = 0.5 * (hsl[8] * c.parseval) + tau * hsl[0];     // :44
        if (objective) objective[k - 1] = f;
        if (mses && td) mses[k - 1] = hsl[3] / (double)C;                // :45
        if (times) times[k - 1] = run.seconds();
        double crit;
        if (stopcriterion == 1)
            crit = fabs(f - obj_prev) / f;                               // :51
        else if (stopcriterion == 2)
            crit = sqrt(hsl[2]) / sqrt(hsl[1]);                          // :53 (0 / 0 = NaN at x = 0: never below the tolerance)
        else
            crit = f;                                                    // :55
        obj_prev = f;
        stop = crit < tolerance;                                         // :64
        return 0;
    };
    int last = 1;
    SBTV_TRY(pipelined_loop(ctx, &last, maxiters, lag, false, enqueue, process, [&] { return !stop; }));
    SBTV_TRY(run.finish(P, last, nullptr, nullptr));
    SBTV_HIP(ctx, hipMemcpyAsync(xw_out_dev, xb[last & 1], sizeof(double) * C, hipMemcpyDeviceToDevice, ctx->stream));
    if (x_out_dev)
        SBTV_HIP(ctx, hipMemcpyAsync(x_out_dev, zb[last & 1], sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// item b of a batch as its solver sees it (device pointers)
struct AdmmItem {
    const double *y, *mask, *tru, *x_init;
    double *x;
};

// What sbtv_CSALSA_v2, sbtv_CoRAL_v2 and sbtv_SALSA_masked do once their arguments are checked.  Independent images go to
// the lanes of this context (`sharded`, group.hip) when it has them.  Else the arrays are staged and the images solved one
// after another by one(b, item, spec): optimistic prox launches first (unless bit 1 of `speculate` asks for exact ones),
// exact ones if the rule fired early.
template <class Sharded, class One>
int admm_batch(sbtv_ctx *ctx, int M, int N, int batch, const sbtv_salsa_opts *opts, const double *y, const double *mask,
               const double *true_x, const double *x_init, double *x_out, int flags, Sharded &&sharded, One &&one) {
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    if (sbtv_group *lg = lanes_group(ctx, batch, false)) {
        LaneCall lc(ctx, lg);
        return lc.done(sharded(lg), batch);
    }
    const size_t P = (size_t)M * N, cnt = P * batch;
    const double *yd = nullptr, *md = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "admm.in.mask", mask, cnt, flags, &md));
    SBTV_TRY(stage_in(ctx, "admm.in.true", true_x, cnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "admm.in.xinit", x_init, cnt, flags, &xi));
    double *xo = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, cnt, flags, &xo));
    for (int b = 0; b < batch; ++b) {
        const size_t o = (size_t)b * P;
        const AdmmItem it{yd + o, off(md, o), off(td, o), off(xi, o), xo + o};
        SBTV_TRY(solve_with_exact_repeat(ctx, !(opts->speculate & 2), [&](bool spec) { return one(b, it, spec); }));
    }
    SBTV_TRY(stage_out_copy(ctx, x_out, xo, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

}  // namespace
}  // namespace sbtv

using namespace sbtv;

extern "C" {

int sbtv_CSALSA_v2(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                   const double *mu1, const double *mu2, const double *sigma, const double *epsilon,
                   double continuationfactor, const sbtv_salsa_opts *opts, const double *true_x, const double *x_init,
                   double *x_out, double *objective, double *distance1, double *distance2, double *criterion,
                   double *times, double *mses, int *numA, int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "CSALSA_v2", y, taps, opts, x_init, M, N, batch, taille));
    if (!mu1 || !mu2 || !sigma) return fail(ctx, SBTV_ERR_BADARG, "CSALSA_v2: missing required argument");
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0))
            return fail(ctx, SBTV_ERR_MISSING_LS, "(A^T A + mu I)^(-1) must be specified: mu1, mu2 must be > 0");
    const size_t t2 = (size_t)taille * taille;
    return admm_batch(
        ctx, M, N, batch, opts, y, nullptr, true_x, x_init, x_out, flags,
        [&](sbtv_group *lg) {
            return csalsa_sharded(lg, y, M, N, batch, taps, taille, mu1, mu2, sigma, epsilon, continuationfactor, opts, true_x,
                                  x_init, x_out, objective, distance1, distance2, criterion, times, mses, numA, numAt,
                                  n_outer, flags);
        },
        [&](int b, const AdmmItem &it, bool spec) {
            const size_t r = (size_t)b * opts->maxiter;                  // every trace row has maxiter entries
            return csalsa_one(ctx, it.y, M, N, taps + b * t2, taille, mu1[b], mu2[b], sigma[b], epsilon ? epsilon[b] : 0.0,
                              continuationfactor, opts, it.tru, it.x_init, it.x, off(objective, r), off(distance1, r),
                              off(distance2, r), off(criterion, r), off(times, r), off(mses, r), off(numA, b), off(numAt, b),
                              off(n_outer, b), spec);
        });
}

int sbtv_CoRAL_v2(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                  const double *tau1, const double *tau2, const double *mu1, const double *mu2, const double *mu_ls,
                  int TViters2, const sbtv_salsa_opts *opts, const double *true_x, const double *x_init, double *x_out,
                  double *objective, double *distance, double *times, double *mses, int *numA, int *numAt, int *n_outer,
                  int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "CoRAL_v2", y, taps, opts, x_init, M, N, batch, taille));
    if (!tau1 || !tau2 || !mu1 || !mu2) return fail(ctx, SBTV_ERR_BADARG, "CoRAL_v2: missing required argument");
    if (TViters2 <= 0) return fail(ctx, SBTV_ERR_MAXITER, "CoRAL_v2: TViters2 must be positive");
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0) || (mu_ls && !(mu_ls[b] > 0.0)))
            return fail(ctx, SBTV_ERR_MISSING_LS, "(A^T A + mu I)^(-1) must be specified: mu1, mu2 must be > 0");
    const size_t t2 = (size_t)taille * taille, mi = (size_t)opts->maxiter;
    return admm_batch(
        ctx, M, N, batch, opts, y, nullptr, true_x, x_init, x_out, flags,
        [&](sbtv_group *lg) {
            return coral_sharded(lg, y, M, N, batch, taps, taille, tau1, tau2, mu1, mu2, mu_ls, TViters2, opts, true_x, x_init,
                                 x_out, objective, distance, times, mses, numA, numAt, n_outer, flags);
        },
        [&](int b, const AdmmItem &it, bool spec) {
            return coral_one(ctx, it.y, M, N, taps + b * t2, taille, tau1[b], tau2[b], mu1[b], mu2[b],
                             mu_ls ? mu_ls[b] : mu1[b] + mu2[b], TViters2, opts, it.tru, it.x_init, it.x,
                             off(objective, b * (mi + 1)), off(distance, b * mi * 2), off(times, b * (mi + 1)),
                             off(mses, b * (mi + 1)), off(numA, b), off(numAt, b), off(n_outer, b), spec);
        });
}

int sbtv_SALSA_masked(sbtv_ctx *ctx, const double *y, const double *mask, int M, int N, int batch, const double *taps,
                      int taille, const double *tau, const double *mu1, const double *mu2, const sbtv_salsa_opts *opts,
                      const double *true_x, const double *x_init, double *x_out, double *objective, double *distance,
                      double *times, double *mses, int *numA, int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "SALSA_masked", y, taps, opts, x_init, M, N, batch, taille));
    if (!mask) return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked: the mask is missing");
    if (!tau || !mu1 || !mu2) return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked: missing required argument");
    for (int b = 0; b < batch; ++b)
        if (!(mu1[b] > 0.0) || !(mu2[b] > 0.0)) return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked: mu1, mu2 must be > 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    const size_t P = (size_t)M * N, cnt = P * batch;
    if (!(flags & SBTV_DEVICE_PTRS))
        for (size_t i = 0; i < cnt; ++i)
            if (!(mask[i] >= 0.0) || std::isinf(mask[i]))
                return fail(ctx, SBTV_ERR_BADARG, "SALSA_masked: the mask must be finite and non-negative");
    const size_t t2 = (size_t)taille * taille, mi = (size_t)opts->maxiter;
    return admm_batch(
        ctx, M, N, batch, opts, y, mask, true_x, x_init, x_out, flags,
        [&](sbtv_group *lg) {
            return masked_sharded(lg, y, mask, M, N, batch, taps, taille, tau, mu1, mu2, opts, true_x, x_init, x_out, objective,
                                  distance, times, mses, numA, numAt, n_outer, flags);
        },
        [&](int b, const AdmmItem &it, bool spec) {
            return masked_one(ctx, it.y, it.mask, M, N, taps + b * t2, taille, tau[b], mu1[b], mu2[b], opts, it.tru, it.x_init,
                              it.x, off(objective, b * (mi + 1)), off(distance, b * mi * 2), off(times, b * (mi + 1)),
                              off(mses, b * (mi + 1)), off(numA, b), off(numAt, b), off(n_outer, b), spec);
        });
}

int sbtv_SALSA_wavelet(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                       const double *h, int hlen, int levels, const double *tau, const double *mu,
                       const sbtv_salsa_opts *opts, const double *true_xw, const double *xw_init, double *xw_out,
                       double *x_out, double *objective, double *distance, double *times, double *mses, int *numA,
                       int *numAt, int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "SALSA_wavelet", y, taps, opts, xw_init, M, N, batch, taille, "xw_init", false));   // no TV prox
    if (!tau || !mu || !xw_out) return fail(ctx, SBTV_ERR_BADARG, "SALSA_wavelet: missing required argument");
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    for (int b = 0; b < batch; ++b)
        if (!(mu[b] > 0.0)) return fail(ctx, SBTV_ERR_BADARG, "SALSA_wavelet: mu must be > 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    const size_t P = (size_t)M * N, C = P * wp.bands(), cnt = P * batch, ccnt = C * batch;
    const double *yd = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "wav.in.true", true_xw, ccnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "wav.in.xinit", xw_init, ccnt, flags, &xi));
    double *xwo = nullptr, *xo = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "wav.out.xw", xw_out, ccnt, flags, &xwo));
    if (x_out) SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, cnt, flags, &xo));
    const size_t mi = (size_t)opts->maxiter;
    for (size_t b = 0; b < (size_t)batch; ++b)
        SBTV_TRY(wavelet_one(ctx, yd + b * P, M, N, taps + b * taille * taille, taille, wp, tau[b], mu[b], opts, off(td, b * C),
                             off(xi, b * C), xwo + b * C, off(xo, b * P), off(objective, b * (mi + 1)), off(distance, b * mi),
                             off(times, b * (mi + 1)), off(mses, b * (mi + 1)), off(numA, b), off(numAt, b), off(n_outer, b)));
    SBTV_TRY(stage_out_copy(ctx, xw_out, xwo, ccnt, flags));
    if (x_out) SBTV_TRY(stage_out_copy(ctx, x_out, xo, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

int sbtv_SALSA_analysis(sbtv_ctx *ctx, const double *y, int M, int N, int batch, const double *taps, int taille,
                        const double *h, int hlen, int levels, const double *tau, const double *mu,
                        const sbtv_salsa_opts *opts, const double *true_x, const double *x_init, double *x_out,
                        double *objective, double *distance, double *times, double *mses, int *numA, int *numAt,
                        int *n_outer, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    SBTV_TRY(check_common(ctx, "SALSA_analysis", y, taps, opts, x_init, M, N, batch, taille, "x_init", false));   // no TV prox
    if (!tau || !mu || !x_out) return fail(ctx, SBTV_ERR_BADARG, "SALSA_analysis: missing required argument");
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    for (int b = 0; b < batch; ++b)
        if (!(mu[b] > 0.0)) return fail(ctx, SBTV_ERR_BADARG, "SALSA_analysis: mu must be > 0");
    SBTV_TRY(check_even_pixels(ctx, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    const size_t P = (size_t)M * N, cnt = P * batch;
    const double *yd = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", y, cnt, flags, &yd));
    SBTV_TRY(stage_in(ctx, "admm.in.true", true_x, cnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "admm.in.xinit", x_init, cnt, flags, &xi));
    double *xo = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, cnt, flags, &xo));
    const size_t mi = (size_t)opts->maxiter;
    for (size_t b = 0; b < (size_t)batch; ++b)
        SBTV_TRY(analysis_one(ctx, yd + b * P, M, N, taps + b * taille * taille, taille, wp, tau[b], mu[b], opts, off(td, b * P),
                              off(xi, b * P), xo + b * P, off(objective, b * (mi + 1)), off(distance, b * mi),
                              off(times, b * (mi + 1)), off(mses, b * (mi + 1)), off(numA, b), off(numAt, b), off(n_outer, b)));
    SBTV_TRY(stage_out_copy(ctx, x_out, xo, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

int sbtv_fista_l1(sbtv_ctx *ctx, const double *b, int M, int N, int batch, const double *taps, int taille, const double *h,
                  int hlen, int levels, const double *tau, double L, int stopcriterion, double tolerance, int maxiters,
                  const double *true_xw, const double *xw_init, double *xw_out, double *x_out, double *objective,
                  double *times, double *mses, int *n_iter, int flags) {
    if (!ctx) return SBTV_ERR_BADARG;
    if (!b || !taps || !h || !tau || !xw_out || batch < 1)
        return fail(ctx, SBTV_ERR_BADARG, "fista_l1: missing required argument (b, taps, h, tau, xw_out; batch >= 1)");
    if (stopcriterion < 1 || stopcriterion > 3) return fail(ctx, SBTV_ERR_STOPCRITERION, "Invalid stopping criterion!");   // :57
    if (maxiters < 1) return fail(ctx, SBTV_ERR_MAXITER, "fista_l1: maxiters must be positive");
    if (!std::isfinite(L) || !(L > 0.0)) return fail(ctx, SBTV_ERR_BADARG, "fista_l1: L must be finite and > 0");
    if (std::isnan(tolerance)) return fail(ctx, SBTV_ERR_BADARG, "fista_l1: tolerance is NaN");
    for (int i = 0; i < batch; ++i)
        if (!std::isfinite(tau[i]) || !(tau[i] >= 0.0)) return fail(ctx, SBTV_ERR_BADARG, "fista_l1: tau must be finite and >= 0");
    SBTV_TRY(check_psf_fits(ctx, taille, M, N));
    WavPlan wp;
    SBTV_TRY(wav_plan(ctx, M, N, h, hlen, levels, true, &wp));
    SBTV_TRY(check_even_pixels(ctx, M, N));
    SBTV_HIP(ctx, hipSetDevice(ctx->device));
    { FftPlan chk; SBTV_TRY(fft_plan(ctx, M, N, 1, &chk)); }
    const size_t P = (size_t)M * N, C = P * wp.bands(), cnt = P * batch, ccnt = C * batch;
    const double *bd = nullptr, *td = nullptr, *xi = nullptr;
    SBTV_TRY(stage_in(ctx, "admm.in.y", b, cnt, flags, &bd));
    SBTV_TRY(stage_in(ctx, "wav.in.true", true_xw, ccnt, flags, &td));
    SBTV_TRY(stage_in(ctx, "wav.in.xinit", xw_init, ccnt, flags, &xi));
    double *xwo = nullptr, *xo = nullptr;
    SBTV_TRY(stage_out_buf(ctx, "wav.out.xw", xw_out, ccnt, flags, &xwo));
    if (x_out) SBTV_TRY(stage_out_buf(ctx, "admm.out.x", x_out, cnt, flags, &xo));
    const size_t mi = (size_t)maxiters;
    const int lag = (flags & SBTV_FISTA_L1_NOLAG) ? 0 : 1;
    for (size_t i = 0; i < (size_t)batch; ++i)
        SBTV_TRY(fista_l1_one(ctx, bd + i * P, M, N, taps + i * taille * taille, taille, wp, tau[i], L, stopcriterion, tolerance,
                              maxiters, lag, off(td, i * C), off(xi, i * C), xwo + i * C, off(xo, i * P), off(objective, i * mi),
                              off(times, i * mi), off(mses, i * mi), off(n_iter, i)));
    SBTV_TRY(stage_out_copy(ctx, xw_out, xwo, ccnt, flags));
    if (x_out) SBTV_TRY(stage_out_copy(ctx, x_out, xo, cnt, flags));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return canary_epilogue(ctx, 0);
}

}  // extern "C"

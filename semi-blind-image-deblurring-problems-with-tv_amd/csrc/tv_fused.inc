// Temporally fused Chambolle kernel body (included by tv.hip inside namespace sbtv).
// See the block comment in tv.hip for the decomposition.
//
// Template knobs
//   FCJ      columns per wave (region = 128 rows x 4 FCJ columns, halo FH on every side)
//   FAST     false: IEEE division / sqrt, no FMA contraction: rounds like the reference's
//                   element-wise MATLAB operations (validation build of the arithmetic)
//            true : one reciprocal per pixel (v_rcp_f64 + ONE cubic correction step, 3 FMAs), rsq-based sqrt
//                   (v_rsq_f64 + a 5-operation refinement) and FMA contraction; every operation
//                   stays within ~1 ulp of the IEEE result (the divisors lie in [1, 1+tau*|grad u|],
//                   no scaling / denormal paths are needed)
//   INTERIOR true for workgroups whose whole region is strictly inside the image: every
//            boundary select of DivergenceIm / GradientIm (:152-166) disappears

#ifndef SBTV_FUSED_SCHED_FREE_MAX_CJ
#define SBTV_FUSED_SCHED_FREE_MAX_CJ 0      // columns-per-wave up to which the scheduler may interleave columns
#endif

// Arithmetic diet of round 3 (profiles/r03_chambolle_diet.md): SBTV_DIET bit 0: the reciprocal by ONE cubic step
// (r0 (1 + e + e^2), e = 1 - d r0: 3 FMAs, error e^3 ~ 2^-70) instead of two Newton steps (4 FMAs); bit 1: the square
// root in 5 operations (see fused_sqrt).  Both stay within ~1 ulp of the IEEE result like the forms they replace.
#ifndef SBTV_DIET
#define SBTV_DIET 3
#endif
__device__ __forceinline__ double fused_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
#if SBTV_DIET & 1
    return __builtin_fma(r, __builtin_fma(e, e, e), r);
#else
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
#endif
}

// sqrt(s) for s >= FUSED_TINY > 0 (the caller adds FUSED_TINY = 1e-300 to the sum of squares: for
// s = 0 the result 1e-150 is indistinguishable from 0 in every use, for s > 1e-284 the sum is
// unchanged, and v_rsq_f64 never sees 0).  v_rsq_f64 (~2^-24 relative) + one Goldschmidt step
// (-> ~2^-47) + one residual correction (-> correctly rounded in all but rare half-ulp cases).
constexpr double FUSED_TINY = 1e-300;
// SBTV_DIET bit 1: with y = rsq(s) (1 + eps), g = s y and e = 1 - g y (one FMA, exact residual of the ROUNDED g, so the
// rounding of g is corrected too): sqrt(s) = g (1 - e)^(-1/2) = g + g e (1/2 + 3/8 e) + O(e^3), e ~ 2^-23: 5 operations
// instead of 8, error ~ 2^-54 + the final rounding.
__device__ __forceinline__ double fused_sqrt(double s) {
    const double y = __builtin_amdgcn_rsq(s);
#if SBTV_DIET & 2
    const double g = s * y;
    const double e = __builtin_fma(-g, y, 1.0);
    const double p = __builtin_fma(0.375, e, 0.5);
    return __builtin_fma(g * e, p, g);
#endif
    double gq = s * y, h = 0.5 * y;
    const double r = __builtin_fma(-gq, h, 0.5);
    gq = __builtin_fma(gq, r, gq);
    h = __builtin_fma(h, r, h);
    const double d = __builtin_fma(-gq, gq, s);     // residual correction
    return __builtin_fma(d, h, gq);
}

//   ESUB     optimistic launches of a solver loop only: the error sum of a step runs over the FIRST column of every wave
//            instead of all of them.  Such a launch does not apply the stop rule; its caller only checks afterwards that
//            the rule cannot have fired before the last step (every step sum > tol^2) and repeats the prox exactly
//            otherwise.  A sum over a subset of the pixels is a lower bound of the full sum, so "subset sum > tol^2"
//            proves the same thing with a quarter of the error arithmetic (10 % of the vector instructions of a step);
//            a subset sum at or below tol^2 takes the exact path like a fired rule does - never a different result.
template <int FCJ, int FNW, bool FAST, bool INTERIOR, bool ESUB = false>
__device__ __forceinline__ void fused_body(const double *__restrict__ gg, const double *__restrict__ pxi,
                                           const double *__restrict__ pyi, double *__restrict__ pxo,
                                           double *__restrict__ pyo, double *__restrict__ partial_out /* + s*nblk */,
                                           int nblk, int M, int N, int ti, int tj, int nsteps, double lambda,
                                           double tau, double *__restrict__ lds_base, double *__restrict__ f_out) {
    constexpr int FRJ = FCJ * FNW;
    // LDS carve-up (one array keeps the compiler from splitting the allocation)
    double(*gl_lds)[FRI] = reinterpret_cast<double(*)[FRI]>(lds_base);                 // [FRJ][FRI]
    double(*ex_u)[FRI] = reinterpret_cast<double(*)[FRI]>(lds_base + FRJ * FRI);       // [FNW][FRI]
    double(*ex_py)[FRI] = reinterpret_cast<double(*)[FRI]>(lds_base + (FRJ + FNW) * FRI);
    // per-lane error sums of every step [FH][64 FNW]: reduced ONCE after the last step (a wave-level reduction inside
    // the step loop is a chain of six dependent LDS round trips right before the barrier every wave has to reach)
    double(*esl)[64 * FNW] = reinterpret_cast<double(*)[64 * FNW]>(lds_base + (FRJ + 2 * FNW) * FRI);   // [FH][64 FNW]

    SBTV_TL(0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rl = 2 * lane;                      // region-local row of .x
    const int gi = ti * FCI - FH + rl;            // global row of .x (even; M is even on this path)
    const int jw = tj * (FRJ - FHL - FHJ) - FHL + w * FCJ;   // global column of this wave's first column
    const bool rin = INTERIOR || ((gi >= 0) && (gi < M));
    const bool rcore = (rl >= FH) && (rl < FRI - FH);
    const double inv_lambda = 1.0 / lambda;

    double2 px[FCJ], py[FCJ];
#pragma unroll
    for (int q = 0; q < FCJ; ++q) {
        const int gj = jw + q;
        const bool in = INTERIOR || (rin && (gj >= 0) && (gj < N));
        // (clamped address + select instead of a branch per column: the loads of all columns are then issued together;
        // gi is even and M is even on this path, so gi in range implies gi + 1 in range)
        const int gjc = min(max(gj, 0), N - 1), gic = min(max(gi, 0), M - 2);
        double2 cc = *reinterpret_cast<const double2 *>(gg + (size_t)gjc * M + gic);
        if (FAST) {
            cc.x = cc.x * inv_lambda;              // g/lambda (:124) as g * (1/lambda): <= 1 ulp from the quotient
            cc.y = cc.y * inv_lambda;
        } else {
            cc.x = cc.x / lambda;                  // IEEE division, once per launch
            cc.y = cc.y / lambda;
        }
        if (!in) cc = make_double2(0.0, 0.0);
        *reinterpret_cast<double2 *>(&gl_lds[w * FCJ + q][rl]) = cc;   // only this lane reads it back
        if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int q = 0; q < FCJ; ++q) {
        const int gj = jw + q;
        const bool in = INTERIOR || (rin && (gj >= 0) && (gj < N));
        double2 a = make_double2(0.0, 0.0), bb = a;
        if (pxi) {                                          // pxi == nullptr: cold start, the duals are zero
            const int gjc = min(max(gj, 0), N - 1), gic = min(max(gi, 0), M - 2);
            const size_t off = (size_t)gjc * M + gic;
            a = *reinterpret_cast<const double2 *>(pxi + off);
            bb = *reinterpret_cast<const double2 *>(pyi + off);
            if (!in) {
                a = make_double2(0.0, 0.0);
                bb = a;
            }
        }
        px[q] = a;
        py[q] = bb;
    }
    *reinterpret_cast<double2 *>(&ex_py[w][rl]) = py[FCJ - 1];
    __syncthreads();
    SBTV_TL(1);

    // u = div p - g/lambda for column q of this wave; pyl = py(., column q-1)
    auto load_gl = [&](int q) -> double2 { return *reinterpret_cast<const double2 *>(&gl_lds[w * FCJ + q][rl]); };
    auto compute_u = [&](int q, double2 pyl, double2 glq) -> double2 {
        const double pxm = dpp_from_prev_lane(px[q].y);              // px(gi-1, gj)
        if (INTERIOR) {
            return make_double2(((py[q].x - pyl.x) + (px[q].x - pxm)) - glq.x,
                                ((py[q].y - pyl.y) + (px[q].y - px[q].x)) - glq.y);
        }
        const int gj = jw + q;
        const double dx0 = div1(px[q].x, pxm, gi, M);
        const double dx1 = div1(px[q].y, px[q].x, gi + 1, M);
        const double dy0 = div1(py[q].x, pyl.x, gj, N);
        const double dy1 = div1(py[q].y, pyl.y, gj, N);
        return make_double2((dy0 + dx0) - glq.x, (dy1 + dx1) - glq.y);
    };

#ifndef SBTV_FUSED_SPLIT
#define SBTV_FUSED_SPLIT 1
#endif
#if SBTV_FUSED_SPLIT
    // ---- step loop, split schedule (round 3) ----------------------------------------------------------------------
    // A step has two exchanges with the neighbouring waves: u of the right neighbour's first column (for the gradient in the
    // wave's LAST column) and py of the left neighbour's last column (for u of the wave's FIRST column).  The first
    // schedule did all four columns between the two barriers and only the exchange between the second and the first:
    // ~25 instructions and two dependent LDS round trips with nothing to overlap them, a quarter of a workgroup's
    // iteration time on the timeline (profiles/r03_chambolle_timeline.md).  Here the columns run in DESCENDING order:
    //   after barrier 1 (ex_u visible): column FCJ-1 (the only one that needs the neighbour's u), publish its new py
    //   after barrier 2 (ex_py visible): columns FCJ-2 .. 0 (u of column 0 was formed at the end of the previous step),
    //     then u of column 0 for the NEXT step from the left neighbour's new py (its LDS read was issued right after the
    //     barrier) and publish it.
    // Every LDS round trip now has a column of arithmetic in front of it.  u(q) needs py(q-1) of the OLD iterate: in
    // descending order column q-1 is still untouched when u(q) is formed.
    auto column_step = [&](int q, double2 uc, double2 un, double &esum) {
        const int gj = jw + q;
        const double ud = dpp_from_next_lane(uc.x);              // u(gi+2, gj)
        double upx0, upx1, upy0, upy1;
        if (INTERIOR) {
            upx0 = uc.y - uc.x;
            upx1 = ud - uc.y;
            upy0 = un.x - uc.x;
            upy1 = un.y - uc.y;
        } else {
            const bool jin = (gj < N - 1);
            upx0 = (gi < M - 1) ? (uc.y - uc.x) : 0.0;
            upx1 = (gi + 1 < M - 1) ? (ud - uc.y) : 0.0;
            upy0 = jin ? (un.x - uc.x) : 0.0;
            upy1 = jin ? (un.y - uc.y) : 0.0;
        }
        const int cl = w * FCJ + q;                              // region-local column
        const bool ecore = (!ESUB || q == 0) && rcore && rin && cl >= FHL && cl < FRJ - FHJ && (INTERIOR || (gj >= 0 && gj < N));
        if (FAST) {
#pragma clang fp contract(fast)
            const double t0 = fused_sqrt(upx0 * upx0 + (upy0 * upy0 + FUSED_TINY));
            const double t1 = fused_sqrt(upx1 * upx1 + (upy1 * upy1 + FUSED_TINY));
            if (ecore) {
                const double a0 = t0 * px[q].x - upx0, b0 = t0 * py[q].x - upy0;
                if constexpr (ESUB) {
                    esum += __builtin_fma(b0, b0, a0 * a0);          // (the even rows of the column: a lower bound is all it takes)
                } else {
                    const double a1 = t1 * px[q].y - upx1, b1 = t1 * py[q].y - upy1;
                    // one chain of four fused multiply-adds (a pair-wise tree costs a fifth operation)
                    esum += __builtin_fma(b1, b1, __builtin_fma(a1, a1, __builtin_fma(b0, b0, a0 * a0)));
                }
            }
            const double r0 = fused_rcp(1.0 + tau * t0);
            const double r1 = fused_rcp(1.0 + tau * t1);
            px[q].x = (px[q].x + tau * upx0) * r0;
            px[q].y = (px[q].y + tau * upx1) * r1;
            py[q].x = (py[q].x + tau * upy0) * r0;
            py[q].y = (py[q].y + tau * upy1) * r1;
        } else {
            const double t0 = sqrt(upx0 * upx0 + upy0 * upy0);
            const double t1 = sqrt(upx1 * upx1 + upy1 * upy1);
            if (ecore) {
                const double a0 = -upx0 + t0 * px[q].x, b0 = -upy0 + t0 * py[q].x;
                const double a1 = -upx1 + t1 * px[q].y, b1 = -upy1 + t1 * py[q].y;
                esum += a0 * a0 + b0 * b0;
                esum += a1 * a1 + b1 * b1;
            }
            px[q].x = (px[q].x + tau * upx0) / (1.0 + tau * t0);
            px[q].y = (px[q].y + tau * upx1) / (1.0 + tau * t1);
            py[q].x = (py[q].x + tau * upy0) / (1.0 + tau * t0);
            py[q].y = (py[q].y + tau * upy1) / (1.0 + tau * t1);
        }
    };
    double2 u0;
    {
        const double2 pyl0 = (w > 0) ? *reinterpret_cast<const double2 *>(&ex_py[w - 1][rl]) : make_double2(0.0, 0.0);
        u0 = compute_u(0, pyl0, load_gl(0));
        *reinterpret_cast<double2 *>(&ex_u[w][rl]) = u0;
    }
    SBTV_TLW(0);
    SBTV_TLW(1);
    if (nsteps > 0) __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        SBTV_TLW(2 + 4 * s);
        double esum = 0.0;
        // phase 1: the last column
        double2 un = (w < FNW - 1) ? *reinterpret_cast<const double2 *>(&ex_u[w + 1][rl]) : make_double2(0.0, 0.0);
        double2 uc = (FCJ > 1) ? compute_u(FCJ - 1, py[FCJ > 1 ? FCJ - 2 : 0], load_gl(FCJ - 1)) : u0;
        double2 gln = load_gl(FCJ > 2 ? FCJ - 2 : 0);
        column_step(FCJ - 1, uc, un, esum);
        *reinterpret_cast<double2 *>(&ex_py[w][rl]) = py[FCJ - 1];
        __builtin_amdgcn_sched_barrier(0);
        SBTV_TLW(3 + 4 * s);
        __syncthreads();
        SBTV_TLW(4 + 4 * s);
        // the left neighbour's new py: needed only at the end of the step (u of column 0 of the next step)
        const double2 pyl_new = (w > 0) ? *reinterpret_cast<const double2 *>(&ex_py[w - 1][rl]) : make_double2(0.0, 0.0);
        // phase 2: columns FCJ-2 .. 0
#pragma unroll
        for (int q = FCJ - 2; q >= 0; --q) {
            un = uc;
            if (q > 0) {
                const double2 glc = gln;
                if (q > 1) gln = load_gl(q - 1);                     // prefetch one column ahead (descending)
                uc = compute_u(q, py[q - 1], glc);
            } else {
                uc = u0;
            }
            column_step(q, uc, un, esum);
            __builtin_amdgcn_sched_barrier(0);                       // keep the columns sequential: bounds register pressure
        }
        esl[s][threadIdx.x] = esum;
        if (s + 1 < nsteps) {
            u0 = compute_u(0, pyl_new, load_gl(0));
            *reinterpret_cast<double2 *>(&ex_u[w][rl]) = u0;
        }
        SBTV_TLW(5 + 4 * s);
        __syncthreads();
    }
#else
    SBTV_TLW(0);
    for (int s = 0; s < nsteps; ++s) {
        const double2 pyl0 = (w > 0) ? *reinterpret_cast<const double2 *>(&ex_py[w - 1][rl]) : make_double2(0.0, 0.0);
        double2 uc = compute_u(0, pyl0, load_gl(0));
        double2 gln = load_gl(1);                                    // g/lambda of the NEXT column, one column ahead
        *reinterpret_cast<double2 *>(&ex_u[w][rl]) = uc;
        SBTV_TLW(1 + 4 * s);
        __syncthreads();
        SBTV_TLW(2 + 4 * s);
        double esum = 0.0;
#pragma unroll
        for (int q = 0; q < FCJ; ++q) {
            double2 un;
            if (q + 1 < FCJ) {
                const double2 glc = gln;
                if (q + 2 < FCJ) gln = load_gl(q + 2);               // prefetch: its LDS latency hides under this column
                un = compute_u(q + 1, py[q], glc);
            } else {
                un = (w < FNW - 1) ? *reinterpret_cast<const double2 *>(&ex_u[w + 1][rl]) : make_double2(0.0, 0.0);
            }
            const int gj = jw + q;
            const double ud = dpp_from_next_lane(uc.x);              // u(gi+2, gj)
            double upx0, upx1, upy0, upy1;
            if (INTERIOR) {
                upx0 = uc.y - uc.x;
                upx1 = ud - uc.y;
                upy0 = un.x - uc.x;
                upy1 = un.y - uc.y;
            } else {
                const bool jin = (gj < N - 1);
                upx0 = (gi < M - 1) ? (uc.y - uc.x) : 0.0;
                upx1 = (gi + 1 < M - 1) ? (ud - uc.y) : 0.0;
                upy0 = jin ? (un.x - uc.x) : 0.0;
                upy1 = jin ? (un.y - uc.y) : 0.0;
            }
            const int cl = w * FCJ + q;                              // region-local column
            const bool ecore = rcore && rin && cl >= FHL && cl < FRJ - FHJ && (INTERIOR || (gj >= 0 && gj < N));
            if (FAST) {
#pragma clang fp contract(fast)
                const double t0 = fused_sqrt(upx0 * upx0 + (upy0 * upy0 + FUSED_TINY));
                const double t1 = fused_sqrt(upx1 * upx1 + (upy1 * upy1 + FUSED_TINY));
                if (ecore) {
                    const double a0 = t0 * px[q].x - upx0, b0 = t0 * py[q].x - upy0;
                    const double a1 = t1 * px[q].y - upx1, b1 = t1 * py[q].y - upy1;
                    // one chain of four fused multiply-adds (a pair-wise tree costs a fifth operation)
                    esum += __builtin_fma(b1, b1, __builtin_fma(a1, a1, __builtin_fma(b0, b0, a0 * a0)));
                }
                const double r0 = fused_rcp(1.0 + tau * t0);
                const double r1 = fused_rcp(1.0 + tau * t1);
                px[q].x = (px[q].x + tau * upx0) * r0;
                px[q].y = (px[q].y + tau * upx1) * r1;
                py[q].x = (py[q].x + tau * upy0) * r0;
                py[q].y = (py[q].y + tau * upy1) * r1;
            } else {
                const double t0 = sqrt(upx0 * upx0 + upy0 * upy0);
                const double t1 = sqrt(upx1 * upx1 + upy1 * upy1);
                if (ecore) {
                    const double a0 = -upx0 + t0 * px[q].x, b0 = -upy0 + t0 * py[q].x;
                    const double a1 = -upx1 + t1 * px[q].y, b1 = -upy1 + t1 * py[q].y;
                    esum += a0 * a0 + b0 * b0;
                    esum += a1 * a1 + b1 * b1;
                }
                px[q].x = (px[q].x + tau * upx0) / (1.0 + tau * t0);
                px[q].y = (px[q].y + tau * upx1) / (1.0 + tau * t1);
                py[q].x = (py[q].x + tau * upy0) / (1.0 + tau * t0);
                py[q].y = (py[q].y + tau * upy1) / (1.0 + tau * t1);
            }
            uc = un;
#ifndef SBTV_FUSED_SCHED_GROUP
#define SBTV_FUSED_SCHED_GROUP 1      // columns the instruction scheduler may interleave (1: strictly one after the other)
#endif
            if (FCJ > SBTV_FUSED_SCHED_FREE_MAX_CJ && ((q + 1) % SBTV_FUSED_SCHED_GROUP) == 0)
                __builtin_amdgcn_sched_barrier(0);   // keep the columns sequential: bounds register pressure
        }
        *reinterpret_cast<double2 *>(&ex_py[w][rl]) = py[FCJ - 1];
        esl[s][threadIdx.x] = esum;
        SBTV_TLW(3 + 4 * s);
        __syncthreads();
        SBTV_TLW(4 + 4 * s);
    }
#endif
    SBTV_TL(2);
    // store the core (nothing to store for a finish-only pass)
    if (nsteps > 0 && rcore && rin) {
#pragma unroll
        for (int q = 0; q < FCJ; ++q) {
            const int cl = w * FCJ + q;
            const int gj = jw + q;
            if (cl >= FHL && cl < FRJ - FHJ && (INTERIOR || (gj >= 0 && gj < N))) {
                const size_t off = (size_t)gj * M + gi;
                *reinterpret_cast<double2 *>(pxo + off) = px[q];
                *reinterpret_cast<double2 *>(pyo + off) = py[q];
            }
        }
    }
    // f = g - lambda * DivergenceIm(px, py)  (chambolle_prox_TV_stop.m:149) for the core, from the
    // duals that are still in registers (ex_py holds the seam columns after the last barrier)
    if (f_out) {
        const double2 pyl0 = (w > 0) ? *reinterpret_cast<const double2 *>(&ex_py[w - 1][rl]) : make_double2(0.0, 0.0);
        // g of all columns first (clamped address): behind the per-column branch below each load would be waited for alone
        double2 gvv[FCJ];
#pragma unroll
        for (int q = 0; q < FCJ; ++q)
            gvv[q] = *reinterpret_cast<const double2 *>(gg + (size_t)min(max(jw + q, 0), N - 1) * M + min(max(gi, 0), M - 2));
#pragma unroll
        for (int q = 0; q < FCJ; ++q) {
            const int cl = w * FCJ + q;
            const int gj = jw + q;
            const double pxm = dpp_from_prev_lane(px[q].y);          // every lane takes part in the DPP move
            const double2 pyl = (q > 0) ? py[q > 0 ? q - 1 : 0] : pyl0;
            if (rcore && rin && cl >= FHL && cl < FRJ - FHJ && (INTERIOR || (gj >= 0 && gj < N))) {
                double dx0, dx1, dy0, dy1;
                if (INTERIOR) {
                    dx0 = px[q].x - pxm;
                    dx1 = px[q].y - px[q].x;
                    dy0 = py[q].x - pyl.x;
                    dy1 = py[q].y - pyl.y;
                } else {
                    dx0 = div1(px[q].x, pxm, gi, M);
                    dx1 = div1(px[q].y, px[q].x, gi + 1, M);
                    dy0 = div1(py[q].x, pyl.x, gj, N);
                    dy1 = div1(py[q].y, pyl.y, gj, N);
                }
                const size_t off = (size_t)gj * M + gi;
                const double2 gv = gvv[q];
                *reinterpret_cast<double2 *>(f_out + off) =
                    make_double2(gv.x - lambda * (dy0 + dx0), gv.y - lambda * (dy1 + dx1));
            }
        }
    }
    // error partial of step s: wave (s mod FNW) adds the FNW per-lane sums of every lane position in wave order, then the
    // xor tree over the lanes - a fixed order, so the partials are bit-reproducible
    for (int s = w; s < nsteps; s += FNW) {
        double acc = 0.0;
#pragma unroll
        for (int ww = 0; ww < FNW; ++ww) acc += esl[s][ww * 64 + lane];
        const double tot = wave_sum(acc);
        if (lane == 0) fused_store_partial(&partial_out[(size_t)s * nblk], tot);
    }
    SBTV_TL(3);
}

template <int FCJ, int FNW, int MINW, bool FAST, bool ESUB = false>
__global__ __launch_bounds__(64 * FNW, MINW) void chambolle_fused_kernel(const double *__restrict__ g,
                                                                          double *__restrict__ pbuf,
                                                                          ProxCtrl *__restrict__ ctrl,
                                                                          double *__restrict__ partials, int M, int N,
                                                                          int batch, int tiles_i, int nblk,
                                                                          int steps_arg, int redo_mode,
                                                                          double *__restrict__ f_all, int write_f,
                                                                          unsigned *__restrict__ counters,
                                                                          int inline_ctrl, SideJob side,
                                                                          const int *__restrict__ order, FusedStagger stg) {
    // write_f: this launch also stores f = g - lambda div p (the last planned launch and the
    // redo launch).  The redo launch doubles as the finish-only pass (0 steps) when no launch has
    // produced a valid f yet (early stop before the last planned launch).
    constexpr int FRJ = FCJ * FNW;
    const int b = blockIdx.z;
    // the first side.nblocks workgroups of the grid host the collector of the previous outer iteration (SideJob)
    const int nside = side.nblocks;
    if ((int)blockIdx.x < nside) {
        __shared__ double sred[4];
        salsa_collect_block(side.c, nullptr, side.out_addr, side.frozen, 0, side.tags_addr, side.seq, blockIdx.x, b, sred);
        return;
    }
    const ProxCtrl c = ctrl[b];
    // bit 2 of `inline_ctrl`: optimistic launch of a solver loop (prox_iterate_spec).  The launch runs exactly
    // `steps_arg` iterations from dual buffer cur ^ phase ^ parity (bit 8: parity of the launch within its prox, bit 9:
    // parity of the launches of earlier optimistic proxes since `cur` was last written) into the
    // other buffer and files its error partials under steps (inline_ctrl >> 12) & 31 onwards; the iteration counter and
    // the stop rule of the control block are not consulted and nothing in it is written (the caller evaluates the rule
    // over all steps afterwards, keeps the parity, and falls back to the exact
    // path if the rule fired before the last step).  `done` still parks images the caller has frozen.
    // bit 3 (with bit 2): multi-buffer mode of a COLD prox (prox_iterate_mb): launch l reads the dual buffer named in bits
    // 20-23 and writes the one in bits 24-27, so that every launch boundary stays available; chambolle_mb_ctrl_kernel
    // then applies the rule over all steps and, if it stopped at an earlier k, the redo launch re-runs the remaining
    // steps from the boundary before k (`cur` = that buffer, `redo` = the steps) into the buffer of bits 24-27.
    const bool spec = (inline_ctrl & 4) != 0, mb = (inline_ctrl & 8) != 0;
    int nsteps;
    if (spec && !redo_mode) {
        if (c.done) return;
        nsteps = steps_arg;
    } else if (redo_mode) {
        if (c.redo <= 0 && (c.f_valid || !f_all)) return;
        nsteps = c.redo > 0 ? c.redo : 0;
    } else {
        if (c.done) return;
        nsteps = min(steps_arg, c.maxiter - c.k);
        if (nsteps <= 0) return;
    }
    const size_t P = (size_t)M * N;
    const size_t plane = P * batch;
    // bit 1 of `inline_ctrl`: cold start (px = py = 0, chambolle_prox_TV_stop.m:68-69) - as long as no iteration
    // has been booked (k == 0: the first launch, or the re-run of an over-run first launch) the duals are
    // not read from memory, so the caller does not have to clear the buffer either
    const bool cold = (inline_ctrl & 2) && (mb && redo_mode ? (c.cur == 0) : spec ? (((inline_ctrl >> 12) & 31) == 0) : (c.k == 0));
    const int src = mb ? (redo_mode ? c.cur : ((inline_ctrl >> 20) & 15)) : ((c.cur ^ (spec ? ((inline_ctrl >> 8) ^ (inline_ctrl >> 9)) : 0)) & 1);
    const int dst = mb ? ((inline_ctrl >> 24) & 15) : (src ^ 1);
    const double *pxi = cold ? nullptr : pbuf + (size_t)(src * 2 + 0) * plane + (size_t)b * P;
    const double *pyi = cold ? nullptr : pbuf + (size_t)(src * 2 + 1) * plane + (size_t)b * P;
    double *pxo = pbuf + (size_t)(dst * 2 + 0) * plane + (size_t)b * P;
    double *pyo = pbuf + (size_t)(dst * 2 + 1) * plane + (size_t)b * P;
    const double *gg = g + (size_t)b * P;
    __shared__ __attribute__((aligned(16))) double lds[(FRJ + 2 * FNW) * FRI + FH * 64 * FNW];
    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (bid % 8 names the
    // group sharing one L2), so give each group a CONTIGUOUS chunk of the tile list: neighbouring
    // tiles, which re-read each other's halos, then hit the same L2.  Bijective for any tile count.
    int tile;
    {
        const int nt = gridDim.x - nside, bid = blockIdx.x - nside;
        const int q8 = nt >> 3, r8 = nt & 7, x = bid & 7, o = bid >> 3;
        tile = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + o;
        // with a table (prox_plan): the same chunks, but inside a chunk the slower border tiles come first, so that the
        // last, partly filled round of workgroups consists of interior tiles only
        if (order) tile = order[bid];
    }
    double *fo = (write_f && f_all) ? f_all + (size_t)b * P : nullptr;
    const int stagger = stg.stagger;
    if (stagger > 0) {
        // workgroups 256..511 are the SECOND workgroup of their CU in the first round (blocks are dealt round-robin over the
        // XCDs and then over an XCD's 32 CUs): hold them back so that the two workgroups of a CU alternate between the memory
        // phase and the arithmetic phase instead of sharing both (tv.hip fused_stagger)
        const int bid = blockIdx.x - nside;
        if (bid >= 256 && bid < 512 && b == 0)
            for (int q = 0; q < stagger; ++q) __builtin_amdgcn_s_sleep(18);      // ~0.5 us per round
    }
    const int ti = tile % tiles_i, tj = tile / tiles_i;
    double *pout = partials + ((size_t)b * FSTRIDE + (spec ? ((inline_ctrl >> 12) & 31) : 0)) * nblk + (size_t)tj * tiles_i + ti;
    // region strictly inside the image (one pixel of margin for the i-1 / j-1 / i+1 / j+1 rules)?
    const int i0 = ti * FCI - FH, j0 = tj * (FRJ - FHL - FHJ) - FHL;
    const bool interior = (i0 >= 1) && (i0 + FRI <= M - 1) && (j0 >= 1) && (j0 + FRJ <= N - 1);
    if (interior)
        fused_body<FCJ, FNW, FAST, true, ESUB>(gg, pxi, pyi, pxo, pyo, pout, nblk, M, N, ti, tj, nsteps, c.lambda, c.tau, lds,
                                               fo);
    else
        fused_body<FCJ, FNW, FAST, false, ESUB>(gg, pxi, pyi, pxo, pyo, pout, nblk, M, N, ti, tj, nsteps, c.lambda, c.tau,
                                                lds, fo);
    if (!spec && ((inline_ctrl & 1) || redo_mode))
        fused_inline_ctrl(&ctrl[b], partials + (size_t)b * FSTRIDE * nblk, nblk, nsteps, write_f, counters + b, redo_mode);
}

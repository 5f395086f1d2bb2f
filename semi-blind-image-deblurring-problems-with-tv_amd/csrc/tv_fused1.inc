// One-row-per-lane variant of the temporally fused Chambolle kernel (included by tv.hip).
//
// Same algorithm as tv_fused.inc, but a lane owns ONE row of FCJ columns instead of a row pair:
// region = 64 rows x (FNW*FCJ) columns, halo 6 rows above / 5 below, 6 columns left / 5 right.
// The per-lane state is half as large (FCJ doubles each of px, py), so the kernel fits in <= 80
// VGPRs and THREE 8-wave workgroups share a CU: while one workgroup streams its region in or out,
// the other two keep the fp64 pipes busy.  Loads are 8 bytes per lane (no alignment requirement,
// so odd M works as well).

// (F1RI, F1HT, F1HB, F1CI are defined in tv.hip)

template <int FCJ, int FNW, bool FAST, bool INTERIOR, bool ESUB>
__device__ __forceinline__ void fused1_body(const double *__restrict__ gg, const double *__restrict__ pxi,
                                            const double *__restrict__ pyi, double *__restrict__ pxo,
                                            double *__restrict__ pyo, double *__restrict__ partial_out, int nblk,
                                            int M, int N, int ti, int tj, int nsteps, double lambda, double tau,
                                            double *__restrict__ lds_base, double *__restrict__ f_out) {
    constexpr int FRJ = FCJ * FNW;
    SBTV_TL(0);
    double(*gl_lds)[F1RI] = reinterpret_cast<double(*)[F1RI]>(lds_base);                       // [FRJ][64]
    double(*ex_u)[F1RI] = reinterpret_cast<double(*)[F1RI]>(lds_base + FRJ * F1RI);            // [FNW][64]
    double(*ex_py)[F1RI] = reinterpret_cast<double(*)[F1RI]>(lds_base + (FRJ + FNW) * F1RI);
    // per-lane error sums of every step, reduced once after the last one (see tv_fused.inc)
    double(*esl)[64 * FNW] = reinterpret_cast<double(*)[64 * FNW]>(lds_base + (FRJ + 2 * FNW) * F1RI);   // [FH][64 FNW]

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int gi = ti * F1CI - F1HT + lane;                       // global row of this lane
    const int jw = tj * (FRJ - FHL - FHJ) - FHL + w * FCJ;        // global column of this wave's first column
    const bool rin = INTERIOR || ((gi >= 0) && (gi < M));
    const bool rcore = (lane >= F1HT) && (lane < F1RI - F1HB);
    const double inv_lambda = 1.0 / lambda;

    double px[FCJ], py[FCJ];
    double g0[FCJ];      // g itself, kept for f = g - lambda div p at the end (a re-load would cost a memory round trip)
#pragma unroll
    for (int q = 0; q < FCJ; ++q) {
        const int gj = jw + q;
        const bool in = INTERIOR || (rin && (gj >= 0) && (gj < N));
        // (clamped address + select instead of a branch per column: the loads of all columns are then issued together;
        // behind per-column branches a border tile waits for one memory round trip per column)
        const int gjc = min(max(gj, 0), N - 1), gic = min(max(gi, 0), M - 1);
        const size_t off = (size_t)gjc * M + gic;
        double a = 0.0, bb = 0.0;
        if (pxi) {                                                 // nullptr: cold start, the duals are zero
            a = pxi[off];
            bb = pyi[off];
        }
        double cc = gg[off];
        g0[q] = cc;
        cc = FAST ? cc * inv_lambda : cc / lambda;                // g/lambda (:124)
        if (!in) {
            a = 0.0;
            bb = 0.0;
            cc = 0.0;
        }
        px[q] = a;
        py[q] = bb;
        gl_lds[w * FCJ + q][lane] = cc;
    }
    ex_py[w][lane] = py[FCJ - 1];
    __syncthreads();
    SBTV_TL(1);

    auto compute_u = [&](int q, double pyl, double glq) -> double {
        const double pxm = dpp_from_prev_lane(px[q]);              // px(gi-1, gj)
        if (INTERIOR) return ((py[q] - pyl) + (px[q] - pxm)) - glq;
        return (div1(py[q], pyl, jw + q, N) + div1(px[q], pxm, gi, M)) - glq;
    };

    for (int s = 0; s < nsteps; ++s) {
        const double pyl0 = (w > 0) ? ex_py[w - 1][lane] : 0.0;
        double uc = compute_u(0, pyl0, gl_lds[w * FCJ][lane]);
        double gln = gl_lds[w * FCJ + (FCJ > 1 ? 1 : 0)][lane];
        ex_u[w][lane] = uc;
        __syncthreads();
        double esum = 0.0;
#pragma unroll
        for (int q = 0; q < FCJ; ++q) {
            double un;
            if (q + 1 < FCJ) {
                const double glc = gln;
                if (q + 2 < FCJ) gln = gl_lds[w * FCJ + q + 2][lane];
                un = compute_u(q + 1, py[q], glc);
            } else {
                un = (w < FNW - 1) ? ex_u[w + 1][lane] : 0.0;
            }
            const int gj = jw + q;
            const double ud = dpp_from_next_lane(uc);               // u(gi+1, gj)
            double upx, upy;
            if (INTERIOR) {
                upx = ud - uc;
                upy = un - uc;
            } else {
                upx = (gi < M - 1) ? (ud - uc) : 0.0;               // GradientIm (:161-166)
                upy = (gj < N - 1) ? (un - uc) : 0.0;
            }
            const int cl = w * FCJ + q;
            // (ESUB: the error sum of an optimistic launch over the first column of every wave only, see tv_fused.inc)
            const bool ecore = (!ESUB || q == 0) && rcore && rin && cl >= FHL && cl < FRJ - FHJ && (INTERIOR || (gj >= 0 && gj < N));
            if (FAST) {
#pragma clang fp contract(fast)
                const double t = fused_sqrt(upx * upx + (upy * upy + FUSED_TINY));
                if (ecore) {
                    const double a0 = t * px[q] - upx, b0 = t * py[q] - upy;
                    esum += a0 * a0 + b0 * b0;
                }
                const double r = fused_rcp(1.0 + tau * t);
                px[q] = (px[q] + tau * upx) * r;
                py[q] = (py[q] + tau * upy) * r;
            } else {
                const double t = sqrt(upx * upx + upy * upy);
                if (ecore) {
                    const double a0 = -upx + t * px[q], b0 = -upy + t * py[q];
                    esum += a0 * a0 + b0 * b0;
                }
                px[q] = (px[q] + tau * upx) / (1.0 + tau * t);
                py[q] = (py[q] + tau * upy) / (1.0 + tau * t);
            }
            uc = un;
        }
        ex_py[w][lane] = py[FCJ - 1];
        esl[s][threadIdx.x] = esum;
        __syncthreads();
    }
    SBTV_TL(2);
    if (nsteps > 0 && rcore && rin) {
#pragma unroll
        for (int q = 0; q < FCJ; ++q) {
            const int cl = w * FCJ + q;
            const int gj = jw + q;
            if (cl >= FHL && cl < FRJ - FHJ && (INTERIOR || (gj >= 0 && gj < N))) {
                const size_t off = (size_t)gj * M + gi;
                pxo[off] = px[q];
                pyo[off] = py[q];
            }
        }
    }
    if (f_out) {
        const double pyl0 = (w > 0) ? ex_py[w - 1][lane] : 0.0;
        // g of all columns first (clamped address): behind the per-column branch below each load would be waited for alone
        double gv[FCJ];
#pragma unroll
        for (int q = 0; q < FCJ; ++q)
            gv[q] = gg[(size_t)min(max(jw + q, 0), N - 1) * M + min(max(gi, 0), M - 1)];
#pragma unroll
        for (int q = 0; q < FCJ; ++q) {
            const int cl = w * FCJ + q;
            const int gj = jw + q;
            const double pxm = dpp_from_prev_lane(px[q]);
            const double pyl = (q > 0) ? py[q > 0 ? q - 1 : 0] : pyl0;
            if (rcore && rin && cl >= FHL && cl < FRJ - FHJ && (INTERIOR || (gj >= 0 && gj < N))) {
                const double dx = INTERIOR ? (px[q] - pxm) : div1(px[q], pxm, gi, M);
                const double dy = INTERIOR ? (py[q] - pyl) : div1(py[q], pyl, gj, N);
                const size_t off = (size_t)gj * M + gi;
                f_out[off] = g0[q] - lambda * (dy + dx);           // (:149)
            }
        }
    }
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
__global__ __launch_bounds__(64 * FNW, MINW) void chambolle_fused1_kernel(const double *__restrict__ g,
                                                                           double *__restrict__ pbuf,
                                                                           ProxCtrl *__restrict__ ctrl,
                                                                           double *__restrict__ partials, int M,
                                                                           int N, int batch, int tiles_i, int nblk,
                                                                           int steps_arg, int redo_mode,
                                                                           double *__restrict__ f_all, int write_f,
                                                                           unsigned *__restrict__ counters,
                                                                           int inline_ctrl, SideJob side) {
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
    __shared__ double lds[(FRJ + 2 * FNW) * F1RI + FH * 64 * FNW];
    int tile;
    {
        const int nt = gridDim.x - nside, bid = blockIdx.x - nside;
        const int q8 = nt >> 3, r8 = nt & 7, x = bid & 7, o = bid >> 3;
        tile = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + o;
    }
    const int ti = tile % tiles_i, tj = tile / tiles_i;
    double *pout = partials + ((size_t)b * FSTRIDE + (spec ? ((inline_ctrl >> 12) & 31) : 0)) * nblk + (size_t)tj * tiles_i + ti;
    const int i0 = ti * F1CI - F1HT, j0 = tj * (FRJ - FHL - FHJ) - FHL;
    const bool interior = (i0 >= 1) && (i0 + F1RI <= M - 1) && (j0 >= 1) && (j0 + FRJ <= N - 1);
    double *fo = (write_f && f_all) ? f_all + (size_t)b * P : nullptr;
    if (interior)
        fused1_body<FCJ, FNW, FAST, true, ESUB>(gg, pxi, pyi, pxo, pyo, pout, nblk, M, N, ti, tj, nsteps, c.lambda, c.tau,
                                                lds, fo);
    else
        fused1_body<FCJ, FNW, FAST, false, ESUB>(gg, pxi, pyi, pxo, pyo, pout, nblk, M, N, ti, tj, nsteps, c.lambda, c.tau,
                                                 lds, fo);
    if (!spec && ((inline_ctrl & 1) || redo_mode))
        fused_inline_ctrl(&ctrl[b], partials + (size_t)b * FSTRIDE * nblk, nblk, nsteps, write_f, counters + b, redo_mode);
}

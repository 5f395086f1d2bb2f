// Blur operator for ARBITRARY image sizes (included by fft.hip inside namespace sbtv).
//
// The reference's closures work for any M x N (utils/resize.m:1-12 pads the kernel into an array of the image's
// size, run_Gaussian_demo.m:136-139 are plain fft2 / ifft2).  The tuned kernels above need powers of two; every other
// size (2 <= M, N <= 4096, not both a supported power of two) takes this path: a full complex 2-D DFT by the chirp-z
// (Bluestein) identity on top of a power-of-two transform of length L >= 2 n - 1,
//     X[k] = c[k] * sum_j (x[j] c[j]) conj(c)[k - j],   c[j] = exp(-+ i pi j^2 / n),
// one workgroup per line with the whole length-L line in LDS: multiply by the chirp, zero-pad, forward radix-2
// decimation-in-frequency transform (natural order in, bit-reversed out), multiply with the pre-computed spectrum of
// the chirp filter (stored bit-reversed), inverse decimation-in-time transform (bit-reversed in, natural out),
// multiply by the chirp.  Correctness path, not a tuned one: ~4 x the work of a power-of-two transform.
//
// Layout in this mode ("generic"): S is the FULL complex spectrum, column-major M x N (pl.n1 = M, pl.s_img = M N);
// operator spectra U likewise (pl.u_img = M N).  The row pass degenerates into the point-wise spectral operator, the
// two column passes carry the whole 2-D transform, and the SALSA bookkeeping is its own element-wise kernel.

struct AnyAxis {           // Bluestein tables of one transform length (device pointers, cached in the context)
    int n, L, logL;
    const double2 *chirp;  // c[j], j < n (forward sign)
    const double2 *Bf;     // FFT_L of the forward chirp filter, bit-reversed order
    const double2 *Bi;     // the same for the inverse transform
    const double2 *twL;    // exp(-2 pi i k / L), k < L
};

constexpr int ANY_THREADS = 256;

// One line per workgroup.  in / out: element e of line q at base + q * line_stride + e * elem_stride.
__global__ __launch_bounds__(ANY_THREADS) void bluestein_lines_kernel(const double2 *__restrict__ in,
                                                                       double2 *__restrict__ out, AnyAxis ax,
                                                                       size_t line_stride, size_t elem_stride,
                                                                       size_t img_stride, int inverse, double scale,
                                                                       const int *__restrict__ frozen) {
    extern __shared__ __attribute__((aligned(16))) double2 any_buf[];
    const int b = blockIdx.y;
    if (frozen && frozen[b]) return;
    const int n = ax.n, L = ax.L;
    const double2 *__restrict__ src = in + (size_t)b * img_stride + (size_t)blockIdx.x * line_stride;
    double2 *__restrict__ dst = out + (size_t)b * img_stride + (size_t)blockIdx.x * line_stride;
    for (int j = threadIdx.x; j < L; j += ANY_THREADS) {
        double2 v = make_double2(0.0, 0.0);
        if (j < n) {
            double2 c = ax.chirp[j];
            if (inverse) c.y = -c.y;
            v = cmul(src[(size_t)j * elem_stride], c);
        }
        any_buf[j] = v;
    }
    __syncthreads();
    // forward transform of length L, decimation in frequency: natural order in, bit-reversed order out
    for (int half = L >> 1, tsh = 0; half >= 1; half >>= 1, ++tsh) {
        for (int idx = threadIdx.x; idx < (L >> 1); idx += ANY_THREADS) {
            const int pos = idx & (half - 1), i = ((idx - pos) << 1) + pos, j = i + half;
            const double2 w = ax.twL[pos << tsh];
            const double2 a = any_buf[i], bb = any_buf[j];
            any_buf[i] = cadd(a, bb);
            any_buf[j] = cmul(csub(a, bb), w);
        }
        __syncthreads();
    }
    const double2 *__restrict__ B = inverse ? ax.Bi : ax.Bf;
    for (int i = threadIdx.x; i < L; i += ANY_THREADS) any_buf[i] = cmul(any_buf[i], B[i]);
    __syncthreads();
    // inverse transform, decimation in time: bit-reversed order in, natural order out
    for (int half = 1, tsh = ax.logL - 1; half < L; half <<= 1, --tsh) {
        for (int idx = threadIdx.x; idx < (L >> 1); idx += ANY_THREADS) {
            const int pos = idx & (half - 1), i = ((idx - pos) << 1) + pos, j = i + half;
            const double2 w = cconj(ax.twL[pos << tsh]);
            const double2 a = any_buf[i], bb = cmul(any_buf[j], w);
            any_buf[i] = cadd(a, bb);
            any_buf[j] = csub(a, bb);
        }
        __syncthreads();
    }
    const double sc = scale / (double)L;
    for (int k = threadIdx.x; k < n; k += ANY_THREADS) {
        double2 c = ax.chirp[k];
        if (inverse) c.y = -c.y;
        dst[(size_t)k * elem_stride] = cscale(cmul(any_buf[k], c), sc);
    }
}

// S = complex(x + add)
__global__ __launch_bounds__(256) void any_real_to_complex_kernel(const double *__restrict__ x,
                                                                   const double *__restrict__ add,
                                                                   double2 *__restrict__ S, size_t P,
                                                                   const int *__restrict__ frozen) {
    const int b = blockIdx.y;
    if (frozen && frozen[b]) return;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < P; q += (size_t)gridDim.x * 256) {
        const size_t o = (size_t)b * P + q;
        S[o] = make_double2(add ? x[o] + add[o] : x[o], 0.0);
    }
}

// point-wise spectral operator over the full spectrum (all Parseval weights are 1); partial sums [b][3][gridDim.x]
template <int OP>
__global__ __launch_bounds__(256) void any_spec_kernel(RowsParams p, size_t P, double2 *__restrict__ outS) {
    constexpr bool needY = (OP == OP_SALSA || OP == OP_RESID || OP == OP_GRAD || OP == OP_GRADF);
    constexpr bool needD = (OP == OP_GRAD);
    __shared__ double red[3 * 4];
    const int b = blockIdx.y;
    if (p.frozen && p.frozen[b]) return;
    const size_t sbase = (size_t)b * P, ubase = p.shared_spec ? 0 : (size_t)b * P;
    const double mu = p.mu ? p.mu[b] : 0.0;
    const double2 z = make_double2(0.0, 0.0);
    double acc[3] = {0.0, 0.0, 0.0};
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < P; q += (size_t)gridDim.x * 256) {
        const double2 r = spec_apply<OP>(p.Sin[sbase + q], p.H[ubase + q], needY ? p.Y[ubase + q] : z,
                                         needD ? p.D1[ubase + q] : z, needD ? p.D2[ubase + q] : z, mu, 1.0, acc);
        if (outS) outS[sbase + q] = r;
    }
    if constexpr (needY) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double a = acc[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
            if (lane == 0) red[c * 4 + w] = a;
        }
        __syncthreads();
        if (threadIdx.x < 3)
            p.acc[((size_t)b * 3 + threadIdx.x) * gridDim.x + blockIdx.x] =
                (red[threadIdx.x * 4] + red[threadIdx.x * 4 + 1]) + (red[threadIdx.x * 4 + 2] + red[threadIdx.x * 4 + 3]);
    }
}

// x = real(S) (already scaled); POST: the SALSA bookkeeping of fft_cols_inv_kernel<., true>, one workgroup per column,
// partial sums [b][6][N]
template <bool POST>
__global__ __launch_bounds__(256) void any_complex_to_real_kernel(const double2 *__restrict__ S, double *__restrict__ x,
                                                                   int M, int N, const int *__restrict__ frozen,
                                                                   ColsPost post) {
    __shared__ double red[6 * 4];
    const int b = blockIdx.y, j = blockIdx.x;
    if (frozen && frozen[b]) return;
    const size_t cb = ((size_t)b * N + j) * M, cl = ((size_t)b * N + (j > 0 ? j - 1 : N - 1)) * M;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < M; i += 256) {
        const double xv = S[cb + i].x;
        x[cb + i] = xv;
        if constexpr (POST) {
            const double uv = post.u[cb + i];
            const double bv = post.bu[cb + i] + (uv - xv);
            post.bu[cb + i] = bv;
            post.g[cb + i] = xv - bv;
            if (post.tru) {
                const double e = xv - post.tru[cb + i];
                acc[0] += e * e;
            }
            const double d = xv - uv;
            acc[1] += d * d;
            acc[2] += xv * xv;
            acc[3] += uv * uv;
            if (post.xprev) {
                const double pd = xv - post.xprev[cb + i];
                acc[4] += pd * pd;
            }
            const double dh = uv - post.u[cl + i], dv = uv - post.u[cb + (i > 0 ? i - 1 : M - 1)];
            acc[5] += sqrt(dh * dh + dv * dv);
        }
    }
    if constexpr (POST) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double a = acc[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
            if (lane == 0) red[c * 4 + w] = a;
        }
        __syncthreads();
        if (threadIdx.x < 6)
            post.partials[((size_t)b * 6 + threadIdx.x) * N + j] =
                (red[threadIdx.x * 4] + red[threadIdx.x * 4 + 1]) + (red[threadIdx.x * 4 + 2] + red[threadIdx.x * 4 + 3]);
    }
}

// spectrum of the zero-padded taps over the full M x N grid (utils/resize.m:1-12), direct DFT
__global__ __launch_bounds__(64) void any_psf_spectrum_kernel(const double *__restrict__ taps, int taille,
                                                               double2 *__restrict__ U, int M, int N,
                                                               const double2 *__restrict__ tw_M,
                                                               const double2 *__restrict__ tw_N) {
    const int b = blockIdx.z, i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= M) return;
    const double *h = taps + (size_t)b * taille * taille;
    double2 acc = make_double2(0.0, 0.0);
    for (int nn = 0; nn < taille; ++nn) {
        double2 cc = make_double2(0.0, 0.0);
        for (int m = 0; m < taille; ++m) {
            const double2 w = tw_M[(int)(((long long)i * m) % M)];
            const double hv = h[nn * taille + m];
            cc.x += hv * w.x;
            cc.y += hv * w.y;
        }
        acc = cadd(acc, cmul(cc, tw_N[(int)(((long long)j * nn) % N)]));
    }
    U[((size_t)b * N + j) * M + i] = acc;
}

// ---- host side ------------------------------------------------------------------------------------------------
// Bluestein length of an n-point line: the next power of two >= 2 n - 1
static inline void any_axis_len(int n, int *L_out, int *logL_out) {
    int L = 1, logL = 0;
    while (L < 2 * n - 1) { L <<= 1; ++logL; }
    *L_out = L;
    *logL_out = logL;
}
static int any_axis_get(sbtv_ctx *ctx, int n, AnyAxis *ax) {
    int L, logL;
    any_axis_len(n, &L, &logL);
    auto it = ctx->any_axes.find(n);
    if (it != ctx->any_axes.end()) {
        const double2 *base = it->second;
        *ax = AnyAxis{n, L, logL, base, base + n, base + n + L, nullptr};
        return twiddle_get(ctx, L, &ax->twL);
    }
    typedef long double ld;
    const ld PI = 3.14159265358979323846264338327950288L;
    std::vector<ld> cr(n), ci(n);
    for (int j = 0; j < n; ++j) {
        const long long r = ((long long)j * j) % (2LL * n);          // exp(-i pi j^2 / n) has period 2 n in j^2
        const ld a = PI * (ld)r / (ld)n;
        cr[j] = cosl(a);
        ci[j] = -sinl(a);
    }
    // chirp filter b[m] = conj(c[|m|]) placed circularly in length L, transformed on the host in long double
    auto fft_host = [&](std::vector<ld> &re, std::vector<ld> &im) {
        for (int i = 1, jj = 0; i < L; ++i) {              // bit reversal
            int bit = L >> 1;
            for (; jj & bit; bit >>= 1) jj ^= bit;
            jj ^= bit;
            if (i < jj) { std::swap(re[i], re[jj]); std::swap(im[i], im[jj]); }
        }
        for (int len = 2; len <= L; len <<= 1) {
            for (int i = 0; i < L; i += len)
                for (int k = 0; k < len / 2; ++k) {
                    const ld a = -2 * PI * (ld)k / (ld)len, wr = cosl(a), wi = sinl(a);
                    const int p0 = i + k, p1 = p0 + len / 2;
                    const ld tr = re[p1] * wr - im[p1] * wi, ti = re[p1] * wi + im[p1] * wr;
                    re[p1] = re[p0] - tr; im[p1] = im[p0] - ti;
                    re[p0] += tr; im[p0] += ti;
                }
        }
    };
    std::vector<double2> host((size_t)n + 2 * L);
    for (int j = 0; j < n; ++j) host[j] = make_double2((double)cr[j], (double)ci[j]);
    for (int dir = 0; dir < 2; ++dir) {
        std::vector<ld> br(L, 0.0L), bi(L, 0.0L);
        for (int m = 0; m < n; ++m) {
            const ld vr = cr[m], vi = dir == 0 ? -ci[m] : ci[m];       // conj(c) forward, c for the inverse transform
            br[m] = vr; bi[m] = vi;
            if (m > 0) { br[L - m] = vr; bi[L - m] = vi; }
        }
        fft_host(br, bi);
        for (int i = 0; i < L; ++i) {                                  // store in bit-reversed order
            int rv = 0;
            for (int q = 0; q < logL; ++q) rv |= ((i >> q) & 1) << (logL - 1 - q);
            host[(size_t)n + (size_t)dir * L + i] = make_double2((double)br[rv], (double)bi[rv]);
        }
    }
    double2 *d = nullptr;
    SBTV_HIP(ctx, hipMalloc((void **)&d, sizeof(double2) * host.size()));
    SBTV_HIP(ctx, hipMemcpy(d, host.data(), sizeof(double2) * host.size(), hipMemcpyHostToDevice));
    ctx->any_axes[n] = d;
    *ax = AnyAxis{n, L, logL, d, d + n, d + n + L, nullptr};
    return twiddle_get(ctx, L, &ax->twL);
}

static int any_fft2(sbtv_ctx *ctx, const FftPlan &pl, double2 *S, int inverse, double scale, const int *frozen) {
    AnyAxis am, an;
    SBTV_TRY(any_axis_get(ctx, pl.M, &am));
    SBTV_TRY(any_axis_get(ctx, pl.N, &an));
    // (per context: the attribute belongs to the DEVICE the function is loaded on, and contexts of one process may sit
    // on different GPUs and run on different host threads)
    bool &attr_done = ctx->any_attr_done;
    if (!attr_done) {      // lines longer than 4096 points need more than the default 64 KB of dynamic LDS
        SBTV_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(bluestein_lines_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * (int)sizeof(double2)));
        attr_done = true;
    }
    const size_t img = (size_t)pl.M * pl.N;
    // columns (contiguous lines), then rows (element stride M); both in place: a workgroup holds its whole line in LDS
    hipLaunchKernelGGL(bluestein_lines_kernel, dim3(pl.N, pl.batch), dim3(ANY_THREADS), sizeof(double2) * am.L,
                       ctx->stream, (const double2 *)S, S, am, (size_t)pl.M, (size_t)1, img, inverse, 1.0, frozen);
    hipLaunchKernelGGL(bluestein_lines_kernel, dim3(pl.M, pl.batch), dim3(ANY_THREADS), sizeof(double2) * an.L,
                       ctx->stream, (const double2 *)S, S, an, (size_t)1, (size_t)pl.M, img, inverse, scale, frozen);
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

static int any_cols_fwd(sbtv_ctx *ctx, const FftPlan &pl, const double *x, const double *add, double2 *S,
                        const int *frozen) {
    const size_t P = (size_t)pl.M * pl.N;
    hipLaunchKernelGGL(any_real_to_complex_kernel, dim3(ew_blocks(P), pl.batch), dim3(256), 0, ctx->stream, x, add, S, P,
                       frozen);
    return any_fft2(ctx, pl, S, 0, 1.0, frozen);
}

static int any_cols_inv(sbtv_ctx *ctx, const FftPlan &pl, const double2 *S, double *x, double scale, const int *frozen,
                        const ColsPost *post) {
    // the inverse transform runs on a copy: callers may use S again
    const size_t P = (size_t)pl.M * pl.N;
    double2 *tmp = nullptr;
    SBTV_TRY(ws_get_t(ctx, "fft.any.tmp", P * pl.batch, &tmp));
    SBTV_HIP(ctx, hipMemcpyAsync(tmp, S, sizeof(double2) * P * pl.batch, hipMemcpyDeviceToDevice, ctx->stream));
    SBTV_TRY(any_fft2(ctx, pl, tmp, 1, scale, frozen));
    if (post)
        hipLaunchKernelGGL(any_complex_to_real_kernel<true>, dim3(pl.N, pl.batch), dim3(256), 0, ctx->stream,
                           (const double2 *)tmp, x, pl.M, pl.N, frozen, *post);
    else
        hipLaunchKernelGGL(any_complex_to_real_kernel<false>, dim3(pl.N, pl.batch), dim3(256), 0, ctx->stream,
                           (const double2 *)tmp, x, pl.M, pl.N, frozen, ColsPost{});
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

constexpr int ANY_SPEC_BLOCKS = 256, ANY_SPEC_THREADS = 256;

static int any_rows(sbtv_ctx *ctx, const FftPlan &pl, const RowsParams &p0, double2 *Sout) {
    RowsParams p = p0;
    const size_t P = (size_t)pl.M * pl.N;
    const dim3 grid(ANY_SPEC_BLOCKS, pl.batch), block(ANY_SPEC_THREADS);
    if (p.op == OP_NONE) {          // the 2-D transforms live in the column passes: nothing to do but a copy
        if (Sout && Sout != p.Sin)
            SBTV_HIP(ctx, hipMemcpyAsync(Sout, p.Sin, sizeof(double2) * P * pl.batch, hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
#define SBTV_ANY_OP(OP_) \
    case OP_: hipLaunchKernelGGL(any_spec_kernel<OP_>, grid, block, 0, ctx->stream, p, P, Sout); break;
    switch (p.op) {
        SBTV_ANY_OP(OP_MUL_H)
        SBTV_ANY_OP(OP_MUL_HC)
        SBTV_ANY_OP(OP_INVLS)
        SBTV_ANY_OP(OP_SALSA)
        SBTV_ANY_OP(OP_RESID)
        SBTV_ANY_OP(OP_GRAD)
        SBTV_ANY_OP(OP_ATA)
        SBTV_ANY_OP(OP_GRADF)
        default: break;
    }
#undef SBTV_ANY_OP
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

static int any_psf_spectrum(sbtv_ctx *ctx, const FftPlan &pl, const double *taps_dev, int taille, double2 *U) {
    hipLaunchKernelGGL(any_psf_spectrum_kernel, dim3((pl.M + 63) / 64, pl.N, pl.batch), dim3(64), 0, ctx->stream, taps_dev,
                       taille, U, pl.M, pl.N, pl.tw_M, pl.tw_N);
    SBTV_HIP(ctx, hipGetLastError());
    return 0;
}

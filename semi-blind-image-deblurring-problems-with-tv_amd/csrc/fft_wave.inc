// Wave-granular FFT passes for the large image sizes (included by fft.hip inside namespace sbtv).
//
// Why a second set of kernels: at 2048 x 2048 one pass has only 8 columns (4 rows) of work per CU, so a kernel
// built from a few big workgroups runs as ONE round of workgroups that all load, then all compute, then all store
// (round 1: 0.40-0.57 of the HBM peak, SQ_WAIT_ANY 67-79 %).  Here the unit of work is as small as the transform
// allows, so that the units sharing a CU drift apart and one unit's arithmetic overlaps its neighbours' memory time:
//   columns : ONE WAVE per column (n1 = M/2 complex points = 64 lanes x V values, V = 16 or 8).  All inter-stage
//             exchanges are wave-local LDS round trips (no workgroup barrier); four waves share a workgroup only to
//             transpose their results through LDS into the tiled spectrum layout (one barrier).
//   rows    : a software-pipelined workgroup of 2 rows x N/8 threads that owns two row pairs and keeps their loads in
//             flight across its arithmetic (rows_pipe_kernel, below).
// Spectrum layout in this mode ("tiled"): S[(l / 4)][k][l % 4] - 64-byte pieces that both the column side (4 columns
// of one k) and the row side (2 rows x 4 values = one 128-byte line) move whole.  Operator spectra (H, Y, D1, D2) are
// tiled the same way, U[(l / 4)][k][l % 4], k = 0..M/2.
//
// The 1-D engine is the same mixed-radix Stockham autosort scheme as in fft.hip, generalised to V values per thread
// and a radix-16 butterfly (two radix-4 layers with the W16 twiddles as constants).

// (TWS, TW, s_tiled() and u_tiled() are defined in fft.hip)

// ---- synchronisation policies of the LDS exchanges
// Wave-local: LDS operations of one wave execute in issue order, so a wave that exchanges data among its own lanes
// needs no hardware barrier - only the compiler must keep the accesses in program order.
struct SyncWave {
    static __device__ __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};
struct SyncBlock {
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};

// exchange buffer of one sequence: interleaved complex values, one pad element per 16 (stage writes have a lane
// stride of 16 elements; 17 x 16 B = 68 banks keeps the 8-lane groups of ds_write_b128 on distinct banks)
template <class SYNC>
struct XSeq {
    double2 *buf;
    static __device__ __forceinline__ int idx(int pos) { return pos + (pos >> 4); }
    static __device__ __forceinline__ void sync() { SYNC::sync(); }
};
// exchange buffer of the pipelined row pass (8 values per thread, 16-lane LDS passes of consecutive threads of one row):
// no padding, the 16-byte slot inside its 256-byte bank row is XOR-swizzled with bits of the row number instead, which
// makes the stage writes of all three exchange patterns (element strides 8, 64 + 1, 1) and the reads conflict-free;
// the one-pad-per-16 layout above leaves the stride-(64 + 1) writes of the second stage with 2-way conflicts
template <class SYNC>
struct XSwz {
    double2 *buf;
    static __device__ __forceinline__ int idx(int pos) {
        const int m = pos >> 4;
        return pos ^ ((m & 7) ^ ((m & 4) << 1));
    }
    static __device__ __forceinline__ void sync() { SYNC::sync(); }
};
// + 2: the regions of the four columns of a tile then start 32 bytes apart modulo the 128-byte bank row, which keeps
// the column-interleaved accesses of the tile transposition on distinct banks
__host__ __device__ constexpr int xseq_elems(int n) { return n + (n >> 4) + 2; }

// ---- radix-16 butterfly: X[4 k1 + k2] = sum_n1 W4^(n1 k1) W16^(n1 k2) sum_n2 W4^(n2 k2) x[n1 + 4 n2]
template <bool INV>
__device__ __forceinline__ double2 mul_w16(double2 a, double wr, double wi) {   // a * (wr + i wi), conjugated for INV
    const double s = INV ? -wi : wi;
    return make_double2(a.x * wr - a.y * s, a.x * s + a.y * wr);
}
template <bool INV>
__device__ __forceinline__ void bfly16(double2 &x0, double2 &x1, double2 &x2, double2 &x3, double2 &x4, double2 &x5,
                                       double2 &x6, double2 &x7, double2 &x8, double2 &x9, double2 &x10, double2 &x11,
                                       double2 &x12, double2 &x13, double2 &x14, double2 &x15) {
    constexpr double C1 = 0.92387953251128675613, S1 = 0.38268343236508977173, R2 = 0.70710678118654752440;
    // layer 1: 4-point transforms over n2 for each n1; afterwards x[n1 + 4 k2] = Y[n1][k2]
    bfly4<INV>(x0, x4, x8, x12);
    bfly4<INV>(x1, x5, x9, x13);
    bfly4<INV>(x2, x6, x10, x14);
    bfly4<INV>(x3, x7, x11, x15);
    // W16^(n1 k2), forward values exp(-2 pi i n1 k2 / 16)
    x5 = mul_w16<INV>(x5, C1, -S1);                       // n1 = 1, k2 = 1 : W^1
    x9 = INV ? make_double2((x9.x - x9.y) * R2, (x9.x + x9.y) * R2)
             : make_double2((x9.x + x9.y) * R2, (x9.y - x9.x) * R2);   // W^2
    x13 = mul_w16<INV>(x13, S1, -C1);                     // W^3
    x6 = INV ? make_double2((x6.x - x6.y) * R2, (x6.x + x6.y) * R2)
             : make_double2((x6.x + x6.y) * R2, (x6.y - x6.x) * R2);   // n1 = 2, k2 = 1 : W^2
    x10 = mul_mi<INV>(x10);                               // W^4 = -i
    x14 = INV ? make_double2((-x14.x - x14.y) * R2, (x14.x - x14.y) * R2)
              : make_double2((x14.y - x14.x) * R2, (-x14.x - x14.y) * R2);   // W^6
    x7 = mul_w16<INV>(x7, S1, -C1);                       // n1 = 3, k2 = 1 : W^3
    x11 = INV ? make_double2((-x11.x - x11.y) * R2, (x11.x - x11.y) * R2)
              : make_double2((x11.y - x11.x) * R2, (-x11.x - x11.y) * R2);   // W^6
    x15 = mul_w16<INV>(x15, -C1, S1);                     // W^9
    // layer 2: 4-point transforms over n1 for each k2; afterwards x[k1 + 4 k2] = X[4 k1 + k2]
    bfly4<INV>(x0, x1, x2, x3);
    bfly4<INV>(x4, x5, x6, x7);
    bfly4<INV>(x8, x9, x10, x11);
    bfly4<INV>(x12, x13, x14, x15);
    // natural order: X[m], m = 4 k1 + k2, sits in x[k1 + 4 k2] - a transposition of the 4 x 4 index square
    double2 t;
    t = x1; x1 = x4; x4 = t;
    t = x2; x2 = x8; x8 = t;
    t = x3; x3 = x12; x12 = t;
    t = x6; x6 = x9; x9 = t;
    t = x7; x7 = x13; x13 = t;
    t = x11; x11 = x14; x14 = t;
}

template <int V, int LR, bool INV>
__device__ __forceinline__ void butterflies_v(double2 (&v)[V]) {
    constexpr int G = V >> LR;
#pragma unroll
    for (int q = 0; q < G; ++q) {
        if constexpr (LR == 4) {
            bfly16<INV>(v[q], v[q + G], v[q + 2 * G], v[q + 3 * G], v[q + 4 * G], v[q + 5 * G], v[q + 6 * G],
                        v[q + 7 * G], v[q + 8 * G], v[q + 9 * G], v[q + 10 * G], v[q + 11 * G], v[q + 12 * G],
                        v[q + 13 * G], v[q + 14 * G], v[q + 15 * G]);
        } else if constexpr (LR == 3) {
            bfly8<INV>(v[q], v[q + G], v[q + 2 * G], v[q + 3 * G], v[q + 4 * G], v[q + 5 * G], v[q + 6 * G],
                       v[q + 7 * G]);
        } else if constexpr (LR == 2) {
            bfly4<INV>(v[q], v[q + G], v[q + 2 * G], v[q + 3 * G]);
        } else {
            bfly2<INV>(v[q], v[q + G]);
        }
    }
}

template <int V, int LOG2N, int LOG2NS, int LR, bool INV, class TW>
__device__ __forceinline__ void twiddles_v(double2 (&v)[V], int t, TW tw) {
    if constexpr (LOG2NS > 0) {
        constexpr int T = (1 << LOG2N) / V;
        constexpr int R = 1 << LR, G = V / R;
        constexpr int SH = LOG2N - LOG2NS - LR;
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const int k = (t + q * T) & ((1 << LOG2NS) - 1);
            if constexpr (R == 16) {
                // 4 table values (w^1, w^2, w^4, w^8), the other 11 powers as products of at most three of them
                // (<= ~3 ulp): 15 table loads per thread would keep 60 registers busy
                const double2 w1 = twid<INV>(tw, k << SH), w2 = twid<INV>(tw, (2 * k) << SH);
                const double2 w4 = twid<INV>(tw, (4 * k) << SH), w8 = twid<INV>(tw, (8 * k) << SH);
                const double2 w3 = cmul(w1, w2), w5 = cmul(w1, w4), w6 = cmul(w2, w4), w7 = cmul(w3, w4);
                v[q + 1 * G] = cmul(v[q + 1 * G], w1);
                v[q + 2 * G] = cmul(v[q + 2 * G], w2);
                v[q + 3 * G] = cmul(v[q + 3 * G], w3);
                v[q + 4 * G] = cmul(v[q + 4 * G], w4);
                v[q + 5 * G] = cmul(v[q + 5 * G], w5);
                v[q + 6 * G] = cmul(v[q + 6 * G], w6);
                v[q + 7 * G] = cmul(v[q + 7 * G], w7);
                v[q + 8 * G] = cmul(v[q + 8 * G], w8);
                v[q + 9 * G] = cmul(v[q + 9 * G], cmul(w1, w8));
                v[q + 10 * G] = cmul(v[q + 10 * G], cmul(w2, w8));
                v[q + 11 * G] = cmul(v[q + 11 * G], cmul(w3, w8));
                v[q + 12 * G] = cmul(v[q + 12 * G], cmul(w4, w8));
                v[q + 13 * G] = cmul(v[q + 13 * G], cmul(w5, w8));
                v[q + 14 * G] = cmul(v[q + 14 * G], cmul(w6, w8));
                v[q + 15 * G] = cmul(v[q + 15 * G], cmul(w7, w8));
            } else {
#pragma unroll
                for (int r = 1; r < R; ++r) v[q + r * G] = cmul(v[q + r * G], twid<INV>(tw, (r * k) << SH));
            }
        }
    }
}

template <int V, int LOG2N, int LOG2NS, int LR, class X>
__device__ __forceinline__ void exchange_v(double2 (&v)[V], int t, const X &x) {
    constexpr int T = (1 << LOG2N) / V;
    constexpr int R = 1 << LR, G = V / R;
#pragma unroll
    for (int q = 0; q < G; ++q) {
        const int j = t + q * T;
        const int k = j & ((1 << LOG2NS) - 1);
        const int j0 = ((j >> LOG2NS) << (LOG2NS + LR)) + k;
#pragma unroll
        for (int r = 0; r < R; ++r) x.buf[X::idx(j0 + (r << LOG2NS))] = v[q + r * G];
    }
    X::sync();
#pragma unroll
    for (int s = 0; s < V; ++s) v[s] = x.buf[X::idx(t + s * T)];
    X::sync();
}

template <int V, int LOG2N, int LOG2NS, bool INV, class X, class TW>
__device__ __forceinline__ void stages_v(double2 (&v)[V], int t, TW tw, const X &x) {
    constexpr int left = LOG2N - LOG2NS;
    constexpr int LV = (V == 16) ? 4 : 3;
    if constexpr (left > 0) {
        constexpr int LR = left >= LV ? LV : left;
        twiddles_v<V, LOG2N, LOG2NS, LR, INV>(v, t, tw);
        butterflies_v<V, LR, INV>(v);
        if constexpr (left - LR > 0) {
            exchange_v<V, LOG2N, LOG2NS, LR>(v, t, x);
            stages_v<V, LOG2N, LOG2NS + LR, INV>(v, t, tw, x);
        }
    }
}

// ---------------------------------------------------------------------------
// column pass, forward: real columns -> tiled packed half spectrum.  One wave per column, four columns per workgroup.
// ---------------------------------------------------------------------------
template <int LOG2N, int V>   // n1 = M/2 = 1 << LOG2N = 64 V
__global__ __launch_bounds__(64 * TW, 2) void cols_fwd_wave_kernel(const double *__restrict__ x,
                                                                 const double *__restrict__ add,
                                                                 double2 *__restrict__ S,
                                                                 const double2 *__restrict__ tw_n1,
                                                                 const double2 *__restrict__ tw_M, int N,
                                                                 const int *__restrict__ frozen,
                                                                 double *__restrict__ tvp) {
    constexpr int n = 1 << LOG2N;
    static_assert(n == 64 * V, "one wave per column");
    constexpr int REG = xseq_elems(n);
    __shared__ __attribute__((aligned(16))) double2 lds[TW * REG];
    const int b = blockIdx.y;
    if (frozen && frozen[b]) return;
    // the wave index as a scalar: column bases then live in SGPRs (saddr + 32-bit lane offset addressing)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tile = blockIdx.x;
    const int j = tile * TW + w;
    const size_t colbase = ((size_t)b * N + j) * n;           // complex elements
    const double2 *__restrict__ xin = reinterpret_cast<const double2 *>(x) + colbase;
    XSeq<SyncWave> X{lds + w * REG};
    double2 v[V];
#pragma unroll
    for (int s = 0; s < V; ++s) v[s] = xin[lane + s * 64];
    if (tvp) {
        // periodic isotropic TV of x (utils/TVnorm.m:2) on the way, one partial sum per column: tvp[b][j].  The row above
        // a lane's first row is the second row of the previous lane (of the previous step for lane 0, of the last
        // element for the very first); the left neighbour column is read once more (it is in L2)
        constexpr int M = 2 * n;
        const double *__restrict__ xl = x + ((size_t)b * N + (j > 0 ? j - 1 : N - 1)) * M;
        double carry = __shfl(v[V - 1].y, 63, 64);                   // x(M-1, j)
        double a = 0.0;
#pragma unroll
        for (int s = 0; s < V; ++s) {
            const double2 ul = *reinterpret_cast<const double2 *>(xl + 2 * (size_t)(lane + s * 64));
            double upv = __shfl_up(v[s].y, 1, 64);
            if (lane == 0) upv = carry;
            carry = __shfl(v[s].y, 63, 64);
            const double h0 = v[s].x - ul.x, v0 = v[s].x - upv, h1 = v[s].y - ul.y, v1 = v[s].y - v[s].x;
            a += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) tvp[(size_t)b * N + j] = a;
    }
    if (add) {
        const double2 *__restrict__ ain = reinterpret_cast<const double2 *>(add) + colbase;
#pragma unroll
        for (int s = 0; s < V; ++s) v[s] = cadd(v[s], ain[lane + s * 64]);
    }
    stages_v<V, LOG2N, 0, false>(v, lane, tw_n1, X);
    SyncWave::sync();
#pragma unroll
    for (int s = 0; s < V; ++s) X.buf[XSeq<SyncWave>::idx(lane + s * 64)] = v[s];
    __syncthreads();
    // real-input split step + coalesced store of the tile: thread -> (k, column) with the column fastest
    double2 *__restrict__ out = S + ((size_t)b * (N >> TWS) + tile) * ((size_t)n << TWS);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int flat = i * (64 * TW) + threadIdx.x;
        const int k = flat >> TWS, c = flat & (TW - 1);
        const double2 *reg = lds + c * REG;
        const double2 Z = reg[XSeq<SyncWave>::idx(k)];
        const double2 Zm = cconj(reg[XSeq<SyncWave>::idx((n - k) & (n - 1))]);
        double2 r;
        if (k == 0) {
            r = make_double2(Z.x + Z.y, Z.x - Z.y);          // X[0] + i X[M/2]
        } else {
            const double2 wv = tw_M[k];
            const double2 su = cadd(Z, Zm), di = csub(Z, Zm);
            const double2 wd = cmul(wv, di);
            r = make_double2(0.5 * (su.x + wd.y), 0.5 * (su.y - wd.x));
        }
        out[flat] = r;
    }
}

// y - a * x with one rounding per operation (what the element-wise gradient-step kernel computes)
__device__ __forceinline__ double2 step_nocontract(double2 y, double a, double2 x) {
#pragma clang fp contract(off)
    const double t0 = a * x.x, t1 = a * x.y;
    return make_double2(y.x - t0, y.y - t1);
}

// column pass, inverse: tiled packed half spectrum -> real columns (times `scale`); POST: + SALSA bookkeeping
// (see fft_cols_inv_kernel).  Partial sums: one per COLUMN (post.partials[b][6][N]).
// PM: 0 plain; 8 gradient step into post.ystep; 16 MYULA step of post.ystep (+ 128: and the running mean / M2 of the
// posterior moments, post.mom); 64 x and post.g = x - post.bu_in; 1 + (2 if post.tru) + (4 if post.xprev): bookkeeping pass (compile-time so that the epilogue is one
// straight-line block the scheduler can software-pipeline)
template <int LOG2N, int V, int PM>
__global__ __launch_bounds__(64 * TW, 2) void cols_inv_wave_kernel(const double2 *__restrict__ S, double *__restrict__ x,
                                                                 const double2 *__restrict__ tw_n1,
                                                                 const double2 *__restrict__ tw_M, int N, double scale,
                                                                 const int *__restrict__ frozen, ColsPost post) {
    constexpr int n = 1 << LOG2N;
    constexpr bool POST = (PM & 1) != 0, HAS_TRU = (PM & 2) != 0, HAS_XPREV = (PM & 4) != 0;
    constexpr bool NOX = (PM & 32) != 0;      // bookkeeping without the x store, bu read from post.bu_in (salsa.hip)
    static_assert(n == 64 * V, "one wave per column");
    constexpr int REG = xseq_elems(n);
    __shared__ __attribute__((aligned(16))) double2 lds[TW * REG];
    const int b = blockIdx.y;
    if (frozen && frozen[b]) return;
    // the wave index as a scalar: column bases then live in SGPRs (saddr + 32-bit lane offset addressing)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tile = blockIdx.x;
    const int j = tile * TW + w;
    const double2 *__restrict__ in = S + ((size_t)b * (N >> TWS) + tile) * ((size_t)n << TWS);
    {
        double2 a[V];
#pragma unroll
        for (int i = 0; i < V; ++i) a[i] = in[i * (64 * TW) + threadIdx.x];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int flat = i * (64 * TW) + threadIdx.x;
            lds[(flat & (TW - 1)) * REG + XSeq<SyncWave>::idx(flat >> TWS)] = a[i];
        }
    }
    __syncthreads();
    XSeq<SyncWave> X{lds + w * REG};
    double2 v[V];
#pragma unroll
    for (int s = 0; s < V; ++s) {
        const int e = lane + s * 64;
        const double2 Xk = X.buf[XSeq<SyncWave>::idx(e)];
        const double2 Xm = cconj(X.buf[XSeq<SyncWave>::idx((n - e) & (n - 1))]);
        if (e == 0) {
            v[s] = make_double2(0.5 * (Xk.x + Xk.y), 0.5 * (Xk.x - Xk.y));          // E + i O
        } else {
            const double2 E = cscale(cadd(Xk, Xm), 0.5);
            const double2 O = cmulc(cscale(csub(Xk, Xm), 0.5), tw_M[e]);
            v[s] = make_double2(E.x - O.y, E.y + O.x);
        }
        // four elements at a time: 16 twiddle loads and 32 LDS reads in flight at once would set the register peak
        if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    SyncWave::sync();
    stages_v<V, LOG2N, 0, true>(v, lane, tw_n1, X);
    const size_t colbase = ((size_t)b * N + j) * n;
    double2 *__restrict__ out = reinterpret_cast<double2 *>(x) + colbase;
    if constexpr (PM == 8) {
        // gradient step y <- y - alpha * x (my_fista.m:25) on the column still in registers; x is not stored.
        // Rounded like the two-pass form (x = scale * v stored, then y - alpha * x without contraction)
        double2 *__restrict__ yp = reinterpret_cast<double2 *>(post.ystep) + colbase;
        double2 yv[V];
#pragma unroll
        for (int s = 0; s < V; ++s) yv[s] = yp[lane + s * 64];
#pragma unroll
        for (int s = 0; s < V; ++s) {
            const double2 xv = cscale(v[s], scale);
            yp[lane + s * 64] = step_nocontract(yv[s], post.alpha, xv);
        }
    } else if constexpr ((PM & ~128) == 16) {
        // MYULA step on the column still in registers (the gradient is never stored): see fft_cols_inv_myula
        if (post.marm.ctrl && blockIdx.x == 0 && threadIdx.x == 0) {
            ProxCtrl c = post.marm.ctrl[b];      // prox_reset(keep_cur = false) for the cold-start prox that follows
            c.k = 0;
            c.done = 0;
            c.cur = 0;
            c.maxiter = post.marm.maxiter;
            c.redo = 0;
            c.f_valid = 0;
            c.err = 0.0;
            c.lambda = post.marm.lambda[b];
            c.tol = post.marm.tol;
            c.tau = post.marm.tau;
            post.marm.ctrl[b] = c;
        }
        double2 *__restrict__ xp = reinterpret_cast<double2 *>(post.ystep) + colbase;
        const double2 *__restrict__ pp = reinterpret_cast<const double2 *>(post.mprox) + colbase;
        const double2 *__restrict__ zp = post.mZ ? reinterpret_cast<const double2 *>(post.mZ) + colbase : nullptr;
        const double s2 = post.msig2[b];
        const unsigned step = post.mrng.step_dev ? (unsigned)post.mrng.step_dev[0] : post.mrng.step;
        const size_t q0 = (size_t)j * n;               // pair index of the column's first row pair within the image
        constexpr bool MOM = (PM & 128) != 0;
        int mk = 0;
        double mrk = 1.0;
        if constexpr (MOM) {
            mk = mom_sample(post.mom);
            mrk = 1.0 / (double)(mk > 0 ? mk : 1);
        }
        constexpr int CH = 4;
#pragma unroll
        for (int c0 = 0; c0 < V; c0 += CH) {
            double2 xv[CH], pv[CH], zv[CH];
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int e = lane + (c0 + q) * 64;
                xv[q] = xp[e];
                pv[q] = pp[e];
                if (zp) zv[q] = zp[e];
            }
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int e = lane + (c0 + q) * 64;
                if (!zp) zv[q] = philox_normal_pair(q0 + e, step, post.mrng.chain0 + (unsigned)b, post.mrng.seed);
                const double2 gv = cscale(v[c0 + q], scale);       // (as the plain pass forms the value it stores)
                double2 r;
                r.x = myula_nocontract(xv[q].x, pv[q].x, gv.x, 1.0, zv[q].x, post.mgam, post.mlamb, s2, post.msq2g);
                r.y = myula_nocontract(xv[q].y, pv[q].y, gv.y, 1.0, zv[q].y, post.mgam, post.mlamb, s2, post.msq2g);
                xp[e] = r;
                // the new sample is still in registers: +32 B per pixel, X is not read again
                if constexpr (MOM)
                    if (mk > 0) moments_pair(post.mom, 2 * (colbase + e), r, mk, mrk);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else if constexpr (PM == 64) {
        // x and g = x - bu (the prox input of C-SALSA, CSALSA_v2.m:476) from the column still in registers
        const double2 *__restrict__ bp = reinterpret_cast<const double2 *>(post.bu_in) + colbase;
        double2 *__restrict__ gp = reinterpret_cast<double2 *>(post.g) + colbase;
        double2 bb[V];
#pragma unroll
        for (int s = 0; s < V; ++s) bb[s] = bp[lane + s * 64];
#pragma unroll
        for (int s = 0; s < V; ++s) {
            const double2 xv = cscale(v[s], scale);
            out[lane + s * 64] = xv;
            gp[lane + s * 64] = make_double2(xv.x - bb[s].x, xv.y - bb[s].y);
        }
    } else if constexpr (!POST) {
#pragma unroll
        for (int s = 0; s < V; ++s) out[lane + s * 64] = cscale(v[s], scale);
    } else {
        constexpr int M = 2 * n;
        const size_t ibase = (size_t)b * N * M;
        const size_t cb = ibase + (size_t)j * M;
        const size_t cl = ibase + (size_t)(j > 0 ? j - 1 : N - 1) * M;   // periodic left neighbour column
        // all five streams of the column as saddr + lane offset; element e = lane + 64 s sits at cb + 2 e
        const double *__restrict__ up_ = post.u + cb + 2 * lane, *__restrict__ ulp = post.u + cl + 2 * lane;
        double *__restrict__ bup = post.bu + cb + 2 * lane, *__restrict__ gp = post.g + cb + 2 * lane;
        const double *__restrict__ bin = NOX ? post.bu_in + cb + 2 * lane : nullptr;   // NOX: another array than bup
        const double *__restrict__ trp = HAS_TRU ? post.tru + cb + 2 * lane : nullptr;
        const double *__restrict__ xpp = HAS_XPREV ? post.xprev + cb + 2 * lane : nullptr;
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        // The bookkeeping streams are fetched CH elements ahead of their use (two register slots): a chunk's loads are
        // in flight while the previous chunk is processed.  u(i-1, j), the upper neighbour for the periodic TV, is the
        // odd row of the previous lane (previous chunk's lane 63 for lane 0; the wrap-around row for the first element).
        constexpr int CH = 2, NCH = V / CH;
        double2 ub[2][CH], bb[2][CH], tb[2][CH], lb[2][CH], xb[2][CH];
        auto fetch = [&](int c, int slot) {
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int off = (c * CH + q) * 128;                 // 64 lanes x 2 doubles per step of s
                ub[slot][q] = *reinterpret_cast<const double2 *>(up_ + off);
                bb[slot][q] = *reinterpret_cast<const double2 *>((NOX ? bin : (const double *)bup) + off);
                lb[slot][q] = *reinterpret_cast<const double2 *>(ulp + off);
                if constexpr (HAS_TRU) tb[slot][q] = nt_load2(trp + off);
                if constexpr (HAS_XPREV) xb[slot][q] = *reinterpret_cast<const double2 *>(xpp + off);
            }
        };
        // (the first fetch must not be hoisted above the last butterfly stage: the transform's registers and two
        // chunks of operands together exceed the 256-register budget and the kernel would spill ~40 registers)
        __builtin_amdgcn_sched_barrier(0);
        double carry = post.u[cb + M - 1];                          // u(M-1, j): upper neighbour of row 0 (periodic)
        fetch(0, 0);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (c + 1 < NCH) fetch(c + 1, (c + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int s = c * CH + q, off = s * 128;
                const double2 xv = cscale(v[s], scale);
                if constexpr (!NOX) nt_store2(reinterpret_cast<double *>(out + lane + s * 64), xv);   // x is not read again in this iteration
                const double2 uv = ub[c & 1][q], ul = lb[c & 1][q];
                double2 bv = bb[c & 1][q];
                bv.x = bv.x + (uv.x - xv.x);
                bv.y = bv.y + (uv.y - xv.y);
                *reinterpret_cast<double2 *>(bup + off) = bv;
                *reinterpret_cast<double2 *>(gp + off) = make_double2(xv.x - bv.x, xv.y - bv.y);
                if constexpr (HAS_TRU) {
                    const double2 tv = tb[c & 1][q];
                    const double e0 = xv.x - tv.x, e1 = xv.y - tv.y;
                    acc[0] += e0 * e0 + e1 * e1;
                }
                const double d0 = xv.x - uv.x, d1 = xv.y - uv.y;
                acc[1] += d0 * d0 + d1 * d1;
                acc[2] += xv.x * xv.x + xv.y * xv.y;
                acc[3] += uv.x * uv.x + uv.y * uv.y;
                if constexpr (HAS_XPREV) {
                    const double2 xo = xb[c & 1][q];
                    const double p0 = xv.x - xo.x, p1 = xv.y - xo.y;
                    acc[4] += p0 * p0 + p1 * p1;
                }
                // periodic isotropic TV of u (utils/TVnorm.m:2)
                double upv = __shfl_up(uv.y, 1, 64);
                if (lane == 0) upv = carry;
                carry = __shfl(uv.y, 63, 64);
                const double h0 = uv.x - ul.x, v0 = uv.x - upv, h1 = uv.y - ul.y, v1 = uv.y - uv.x;
                acc[5] += sqrt(h0 * h0 + v0 * v0) + sqrt(h1 * h1 + v1 * v1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // all six reductions before the one conditional store: with a branch per sum the compiler sinks the whole TV
        // chain (32 square roots, only used by the last sum) below the earlier branches and spills its operands
#pragma unroll
        for (int c = 0; c < 6; ++c) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_xor(acc[c], off, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) post.partials[((size_t)b * 6 + c) * N + j] = acc[c];
        }
    }
}

// ---------------------------------------------------------------------------
// Row pass, software-pipelined (tiled S, column-major operator spectra U[l][k] as in the workgroup row kernel).
// In the loop a row pass runs as ONE round of workgroups from cold HBM, and a workgroup that loads its rows, transforms,
// THEN loads H / Y, applies the operator, transforms back and stores pays four memory latencies and two transfer times
// one after the other (42 us at 2048^2 for 134 MB).  Here a workgroup of 2 rows x N/8 threads (8 values per thread,
// q = row is the fastest thread index so that a wave's accesses to U are 32-byte pieces and to S whole 128-byte lines)
// owns TWO row pairs and keeps loads in flight across its arithmetic:
//     issue S(A), H/Y(A), S(B)  |  FFT(A)  op(A)  issue H/Y(B)  IFFT(A)  store(A)  |  FFT(B)  op(B)  IFFT(B)  store(B)
// Pair A of workgroup w is rows 2w, 2w+1 and pair B rows n1/2 + 2w, n1/2 + 2w + 1: all workgroups together then read
// the first half of every 16 KB k-run of S and U while they are in phase A and the second half in phase B, i.e. the
// chip-wide access stream stays sequential in DRAM (what makes the column-major U the fast layout in the loop,
// profiles/r02_fft_lab.md).  128 registers of operands in flight: one workgroup (8 waves) per CU.
// ---------------------------------------------------------------------------
template <int LOG2N, int OP>
__global__ __launch_bounds__((1 << LOG2N) / 4, 1) void rows_pipe_kernel(RowsParams p) {
    constexpr int N = 1 << LOG2N, V = 8, T = N / V, RK = 2, NT = RK * T, NW = NT / 64;
    constexpr int REG = N;                        // XSwz: no padding
    constexpr bool needH = (OP != OP_NONE);
    constexpr bool CS = (OP == OP_CSALSA);       // state spectrum E in d1[], read and written in place
    constexpr bool needY = (OP == OP_SALSA || OP == OP_RESID || OP == OP_GRADF || OP == OP_GRAD || CS);
    constexpr bool needD = (OP == OP_GRAD);      // four operator spectra: pair B's rows are then not requested ahead
    constexpr bool needD1 = needD || CS, noAhead = needD || CS;
#ifndef SBTV_CS_LATE_Y
#define SBTV_CS_LATE_Y 1
#endif
    // OP_CSALSA at N = 2048: with Y in flight across the transforms like H and E the kernel spills ~46 registers; Y is
    // requested after the forward transform instead (its latency is covered by the row-0 / operator arithmetic only)
    constexpr bool lateY = CS && (SBTV_CS_LATE_Y != 0) && LOG2N == 11;
    __shared__ __attribute__((aligned(16))) double2 lds[RK * REG];
    // the twiddle table lives in LDS: a GLOBAL load issued between a prefetch and its use would have to wait for the
    // prefetched data too (vmcnt counts in order)
    __shared__ __attribute__((aligned(16))) double2 twl_buf[LdsTw::elems(N)];
    const LdsTw twl{twl_buf};
    __shared__ double red[3 * NW];
    // p.fold > 0 (chains that share ONE set of operator spectra): the images are folded into the x dimension of the grid
    // with the image index fastest WITHIN an XCD's share of the row blocks, so that the workgroups of all chains for the
    // same rows run back to back on the same L2 and H / Y / D come from memory once per row block, not once per chain
    const int fold = p.fold;
    const int ntk = fold ? (int)gridDim.x / fold : (int)gridDim.x;     // row blocks per image
    int b = blockIdx.y;
    int kb;
    {
        const int bid = blockIdx.x, xx = bid & 7;
        int o = bid >> 3;
        if (fold) {
            b = o % fold;
            o /= fold;
        }
        const int q8 = ntk >> 3, r8 = ntk & 7;
        kb = (xx < r8 ? xx * (q8 + 1) : r8 * (q8 + 1) + (xx - r8) * q8) + o;
    }
    if (p.frozen && p.frozen[b]) return;
    // lanes 0-31 of a wave work on row q = 0, lanes 32-63 on row q = 1, both on the same 32 columns: a wave's global
    // accesses are then whole 128-byte lines of the tiled layouts (the two rows' 64-byte pieces are adjacent), and every
    // 16-lane group of an LDS instruction stays inside ONE row's exchange buffer, whose padding keeps it conflict-free
    // (with the rows alternating lane by lane, half of the LDS cycles of this kernel were bank conflicts)
    const int q = (threadIdx.x >> 5) & 1, t = (threadIdx.x & 31) | ((threadIdx.x >> 6) << 5);
    const int n1 = p.n1;
    const int k0 = kb * RK + q, k1 = (n1 >> 1) + kb * RK + q;
    const size_t ibase = (size_t)b * n1 * N;
    const double2 *__restrict__ in = p.Sin + ibase;
    double2 *__restrict__ out = p.Sout ? p.Sout + ibase : nullptr;
    XSwz<SyncBlock> X{lds + q * REG};
    const size_t hbase = p.shared_spec ? 0 : (size_t)b * p.u_img;
    const double mu = p.mu ? p.mu[b] : 0.0;
    const double2 z = make_double2(0.0, 0.0);
    // operator spectra, tiled U[(l/4)][k][l%4] or column-major U[l][k]: index = (l/4) 4(n1+1) + (l%4) sb + k sc
    const int sb = p.u_tiled ? 1 : n1 + 1, sc = p.u_tiled ? TW : 1;
    auto uidx = [&](int kk, int l) -> size_t {
        return hbase + (size_t)(l >> TWS) * (TW * (n1 + 1)) + (size_t)((l & (TW - 1)) * sb + kk * sc);
    };
    for (int i = threadIdx.x; i < N; i += NT) twl_buf[LdsTw::idx(i)] = p.tw[i];
    __syncthreads();

    double2 v[V], sn[V], h[V], y[V], d1[needD1 ? V : 1], d2[needD ? V : 1];
    if constexpr (!needD1) d1[0] = z;
    const CsPar cp = CS ? CsPar{p.cs[0], p.cs[1], p.cs[2]} : CsPar{0.0, 0.0, 0.0};
    // every operator application of this kernel: OP_CSALSA goes through its own function (E by reference)
    auto apply = [&](double2 V_, double2 H_, double2 Y_, double2 &E_, double2 D2_, double wgt, double (&acc_)[3]) -> double2 {
        if constexpr (CS) return spec_apply_cs(V_, H_, Y_, E_, mu, cp, wgt, acc_);
        else return spec_apply<OP>(V_, H_, Y_, E_, D2_, mu, wgt, acc_);
    };
    auto dd1 = [&](int s) -> double2 & { return d1[needD1 ? s : 0]; };
    auto dd2 = [&](int s) -> double2 { return needD ? d2[needD ? s : 0] : z; };
#pragma unroll
    for (int s = 0; s < V; ++s) v[s] = in[s_tiled(k0, t + s * T, n1)];
    if constexpr (needH) {
#pragma unroll
        for (int s = 0; s < V; ++s) {
            h[s] = p.H[uidx(k0, t + s * T)];
            if constexpr (needY && !lateY) y[s] = p.Y[uidx(k0, t + s * T)];
            if constexpr (needD) {
                d1[s] = p.D1[uidx(k0, t + s * T)];
                d2[s] = p.D2[uidx(k0, t + s * T)];
            }
            if constexpr (CS) d1[s] = p.E[uidx(k0, t + s * T)];
        }
    }
    if constexpr (!noAhead) {
#pragma unroll
        for (int s = 0; s < V; ++s) sn[s] = in[s_tiled(k1, t + s * T, n1)];
    }
    double acc[3] = {0.0, 0.0, 0.0};

    // ---- pair A
    if (p.fwd) stages_v<V, LOG2N, 0, false>(v, t, twl, X);
    if constexpr (lateY) {
#pragma unroll
        for (int s = 0; s < V; ++s) y[s] = p.Y[uidx(k0, t + s * T)];
    }
    if constexpr (needH) {
        if (kb == 0) {
            // this workgroup owns the packed row 0 = X[0,:] + i X[M/2,:] (thread row q = 0; q = 1 is an ordinary row):
            // un-mix with the mirrored element (through LDS), apply the operator rows 0 and M/2, re-mix
#pragma unroll
            for (int s = 0; s < V; ++s) X.buf[XSwz<SyncBlock>::idx(t + s * T)] = v[s];
            SyncBlock::sync();
#pragma unroll
            for (int s = 0; s < V; ++s) {
                const int l = t + s * T;
                if (q == 0) {
                    const size_t hn = uidx(n1, l);
                    const double2 P = v[s], Q = cconj(X.buf[XSwz<SyncBlock>::idx((N - l) & (N - 1))]);
                    const double2 A = cscale(cadd(P, Q), 0.5);
                    const double2 dB = csub(P, Q);
                    const double2 B = make_double2(0.5 * dB.y, -0.5 * dB.x);   // (P-Q)/(2i)
                    double2 en = needD ? p.D1[hn] : (CS ? p.E[hn] : z);
                    const double2 A2 = apply(A, h[s], needY ? y[s] : z, dd1(s), dd2(s), 1.0, acc);
                    const double2 B2 = apply(B, p.H[hn], needY ? p.Y[hn] : z, en, needD ? p.D2[hn] : z, 1.0, acc);
                    if constexpr (CS) p.E[hn] = en;
                    v[s] = make_double2(A2.x - B2.y, A2.y + B2.x);             // A' + i B'
                } else {
                    v[s] = apply(v[s], h[s], needY ? y[s] : z, dd1(s), dd2(s), 2.0, acc);
                }
                if constexpr (CS) p.E[uidx(k0, t + s * T)] = d1[s];
            }
            SyncBlock::sync();        // the inverse transform re-uses the buffer
        } else {
#pragma unroll
            for (int s = 0; s < V; ++s) {
                v[s] = apply(v[s], h[s], needY ? y[s] : z, dd1(s), dd2(s), 2.0, acc);
                if constexpr (CS) p.E[uidx(k0, t + s * T)] = d1[s];   // (stored at once: the register is free again)
            }
        }
        // pin the running sums here: left to itself the compiler defers the residual arithmetic (only the final
        // reduction needs it) to the end of the kernel and keeps its operands alive in spilled registers
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]));
        // operator spectra of pair B: in flight during the inverse transform and the store of pair A
#pragma unroll
        for (int s = 0; s < V; ++s) {
            h[s] = p.H[uidx(k1, t + s * T)];
            if constexpr (needY && !lateY) y[s] = p.Y[uidx(k1, t + s * T)];
            if constexpr (needD) {
                d1[s] = p.D1[uidx(k1, t + s * T)];
                d2[s] = p.D2[uidx(k1, t + s * T)];
            }
            if constexpr (CS) d1[s] = p.E[uidx(k1, t + s * T)];
        }
    }
    if (p.inv) stages_v<V, LOG2N, 0, true>(v, t, twl, X);
    // (store offsets are re-derived from an opaque copy of t: kept from the loads they would sit in spilled registers)
    int ts = t;
    asm volatile("" : "+v"(ts));
    if (out) {
#pragma unroll
        for (int s = 0; s < V; ++s) out[s_tiled(k0, ts + s * T, n1)] = v[s];
    }
    // ---- pair B
#pragma unroll
    for (int s = 0; s < V; ++s) v[s] = noAhead ? in[s_tiled(k1, t + s * T, n1)] : sn[s];
    if (p.fwd) stages_v<V, LOG2N, 0, false>(v, t, twl, X);
    if constexpr (lateY) {
#pragma unroll
        for (int s = 0; s < V; ++s) y[s] = p.Y[uidx(k1, t + s * T)];
    }
    if constexpr (needH) {
#pragma unroll
        for (int s = 0; s < V; ++s) {
            v[s] = apply(v[s], h[s], needY ? y[s] : z, dd1(s), dd2(s), 2.0, acc);
            if constexpr (CS) p.E[uidx(k1, t + s * T)] = d1[s];
        }
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]));
    }
    if (p.inv) stages_v<V, LOG2N, 0, true>(v, t, twl, X);
    asm volatile("" : "+v"(ts));
    if (out) {
#pragma unroll
        for (int s = 0; s < V; ++s) out[s_tiled(k1, ts + s * T, n1)] = v[s];
    }
    if constexpr (needY) {
        // deterministic workgroup reduction of the accumulators
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_xor(acc[c], off, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c * NW + w] = acc[c];
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            double a = 0.0;
            for (int ww = 0; ww < NW; ++ww) a += red[threadIdx.x * NW + ww];
            p.acc[((size_t)b * 3 + threadIdx.x) * ntk + kb] = a;
        }
    }
}

// ---- layout helpers of the tiled mode -----------------------------------------------------------------------
// plain packed spectrum [l][k] <-> tiled [(l/4)][k][l%4]
__global__ void s_relayout_kernel(const double2 *__restrict__ in, double2 *__restrict__ out, int n1, int N, int to_tiled) {
    const size_t per = (size_t)n1 * N;
    const double2 *ib = in + (size_t)blockIdx.y * per;
    double2 *ob = out + (size_t)blockIdx.y * per;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < per; q += (size_t)gridDim.x * blockDim.x) {
        // q enumerates the TILED order (coalesced on that side)
        const int c = (int)(q & (TW - 1));
        const size_t rest = q >> TWS;
        const int k = (int)(rest % n1), lt = (int)(rest / n1);
        const size_t plain = (size_t)(lt * TW + c) * n1 + k;
        if (to_tiled) ob[q] = ib[plain];
        else ob[plain] = ib[q];
    }
}

// packed tiled S -> operator-spectrum layout of the plan (tiled / column-major U[l][k]), k = 0..n1
__global__ void spec_unpack_tiled_kernel(const double2 *__restrict__ S, double2 *__restrict__ U, int n1, int N, int utiled) {
    const int b = blockIdx.z;
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;       // 0..n1
    if (l >= N) return;
    const double2 *s = S + (size_t)b * n1 * N;
    double2 *u = U + (size_t)b * (n1 + 1) * N;
    double2 r;
    if (k == 0 || k == n1) {
        const double2 P = s[s_tiled(0, l, n1)];
        const double2 Q = cconj(s[s_tiled(0, (N - l) & (N - 1), n1)]);
        if (k == 0) {
            r = cscale(cadd(P, Q), 0.5);
        } else {
            const double2 d = csub(P, Q);
            r = make_double2(0.5 * d.y, -0.5 * d.x);
        }
    } else {
        r = s[s_tiled(k, l, n1)];
    }
    if (utiled) u[u_tiled(k, l, n1)] = r;      // tiled like S (pipelined row kernel)
    else u[(size_t)l * (n1 + 1) + k] = r;      // column-major (workgroup row kernel)
}

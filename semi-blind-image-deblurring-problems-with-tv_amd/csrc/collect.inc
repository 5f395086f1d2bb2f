// The collectors' shared parts (included inside namespace sbtv by sbtv_internal.h users that launch or host them).
// This thread's part of the total of one Chambolle step's error partials pp[0..n) (written by optimistic prox launches):
// the first 256 threads load, in a fixed order; the caller adds the parts up (xor tree, then red[0..3] in pairs).
__device__ __forceinline__ double step_sum_part(const double *pp, int n) {
    double s = 0.0;
    constexpr int NB = 8;
    for (int base = 0; threadIdx.x < 256 && base < n; base += 256 * NB) {
        double v[NB];
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const int q = base + r * 256 + (int)threadIdx.x;
            v[r] = (q < n) ? __hip_atomic_load(pp + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < NB; ++r) s += v[r];
    }
    return s;
}

// The SALSA collector.
// Block qn of image b reduces ONE quantity of SalsaScal in a fixed order (deterministic):
//   qn 0      rows-kernel partials [batch][3][nrb]                          -> resid2 (+ scalar 7: prox iterations booked)
//   qn 1      tvnorm partials (initial objective) or post slot 5             -> tv_u
//   qn 2..6   post-kernel partials [batch][6][npb], slots 0..4               -> mse_num, dist_num, x2, u2, dx2
//   qn 7 + s  error partials of Chambolle step s of an optimistic prox       -> step sums for the host's stop rule
// With rearm = 1 block 0 also re-arms the prox control block for the next outer iteration's warm-started prox
// (k = 0, done = frozen flag, redo = 0, f_valid = 0; lambda / tol / tau / maxiter / cur stay).
// `out`, the step sums and `tags` may point into pinned host memory.  They travel as integers: a POINTER argument to
// coherent host memory makes the runtime end the kernel with a system-scope release; the stores below carry their own
// system-scope ordering.  Runs with the first 256 threads of the workgroup; every thread must call it (barrier inside).
__device__ __forceinline__ void salsa_collect_block(const Collect &c, ProxCtrl *__restrict__ ctrl, unsigned long long out_addr,
                                                    const int *__restrict__ frozen, int rearm, unsigned long long tags_addr,
                                                    double seq, int qn, int b, double *red /* shared [4] */) {
    SalsaScal *__restrict__ out = reinterpret_cast<SalsaScal *>(out_addr);
    double *__restrict__ tags = reinterpret_cast<double *>(tags_addr);
    const bool act = threadIdx.x < 256;
    double s = 0.0;
    if (qn >= 7) {
        s = step_sum_part(c.ppart + ((size_t)b * FSTRIDE + (qn - 7)) * c.pnblk, c.pnblk);
    } else {
        const double *p = nullptr;
        int n = 0;
        if (qn == 0) {
            p = c.acc ? c.acc + ((size_t)b * 3) * c.nrb : nullptr;
            n = c.nrb;
        } else if (qn == 1) {
            if (c.tvp) {
                p = c.tvp + (size_t)b * c.ntv;
                n = c.ntv;
            } else if (c.post) {
                p = c.post + ((size_t)b * 6 + 5) * c.npb;
                n = c.npb;
            }
        } else if (qn == 2 && c.mse0) {
            p = c.mse0 + (size_t)b * 4;        // already a total (pair_sums): one element
            n = 1;
        } else {
            p = c.post ? c.post + ((size_t)b * 6 + (qn - 2)) * c.npb : nullptr;
            n = c.npb;
        }
        if (p && act)
            for (int q = threadIdx.x; q < n; q += 256) s += p[q];
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (act && (threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double total = (red[0] + red[1]) + (red[2] + red[3]);
    if (qn >= 7) {
        reinterpret_cast<double *>(c.psum_addr)[(size_t)b * FSTRIDE + (qn - 7)] = total;
        if (tags) {
            __threadfence_system();
            __hip_atomic_store(&tags[(size_t)b * SALSA_TAGS + 8 + (qn - 7)], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    double *o = reinterpret_cast<double *>(&out[b]);      // SalsaScal is 8 doubles in this order
    o[qn] = total;
    if (qn == 0) {
        o[7] = ctrl ? (double)ctrl[b].k : 0.0;            // Chambolle iterations booked by exact launches
        if (ctrl && rearm) {
            ProxCtrl pc = ctrl[b];
            pc.k = 0;
            pc.done = (frozen && frozen[b]) ? 1 : 0;
            pc.redo = 0;
            pc.f_valid = 0;
            pc.err = 0.0;
            ctrl[b] = pc;
        }
    }
    if (tags) {
        // completion tag of this scalar (pinned, coherent host memory): the host polls the tags instead of waiting for
        // an event - an event record costs the stream 5-6 us of idle time per outer iteration
        __threadfence_system();
        __hip_atomic_store(&tags[(size_t)b * SALSA_TAGS + qn], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (qn == 0) __hip_atomic_store(&tags[(size_t)b * SALSA_TAGS + 7], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// List losses of the ranking train step (include/cffm_hip.h): from the scores of G lists of Lg candidates each, laid
// out [G][Lg] as cffm_expand_candidates_ex orders the rows, the per-list terms, the mean loss and dL/dscore - the dL/dout that
// cffm_backward_dout takes as given.  With t = target[g] and m = Lg - 1:
//
//   BPR       terms[g] = (1/m) sum_{n != t} softplus(s_n - s_t)        dout[n] = sigmoid(s_n - s_t) / (G m),  dout[t] = -sum_{n != t} dout[n]
//   softmax   terms[g] = log sum_n exp(s_n - max) + max - s_t          dout[n] = (p_n - [n = t]) / G
//   loss[0] = (1/G) sum_g terms[g]
//   logQ      the softmax on z_n = s_n - (corr[i_n][0] - corr[i_t][1]) for n != t, z_t = s_t  (cffm_list_loss_logq, further down)
//
// One wavefront per list, walking it in strides of 64; lanes reduce by the xor butterfly (every lane ends with the same value).  The
// loss is summed in two stages in list order - a workgroup's four terms in wave order, then the workgroups' partials by one
// workgroup in a fixed order - so the bits are the same on every run.  Every exponential has a non-positive argument: softplus(x) =
// max(x, 0) + log1p(exp(-|x|)), sigmoid through exp(-|x|), the softmax with its maximum subtracted.
#include "internal.hpp"

#define LL_WAVES 4        // lists per workgroup

__device__ __forceinline__ float ll_wave_sum(float v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float ll_wave_max(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

template <int KIND>
__global__ __launch_bounds__(64 * LL_WAVES) void list_loss_kernel(const float* __restrict__ scores, int G, int Lg,
                                                                  const int32_t* __restrict__ target, float* __restrict__ dout,
                                                                  float* __restrict__ terms, double* __restrict__ part) {
    __shared__ float red[LL_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * LL_WAVES + wave;
    float term = 0.f;                                    // a wavefront past the last list adds an exact zero to its workgroup's partial
    if (g < G) {                                         // wave-uniform
        const float* s = scores + (int64_t)g * Lg;
        float* d = dout + (int64_t)g * Lg;
        const int t = target[g];
        if (t < 0 || t >= Lg) {                          // defined: a zero row and a zero term, s[t] is never formed
            for (int n = lane; n < Lg; n += 64) d[n] = 0.f;
        } else if (KIND == CFFM_LIST_BPR) {
            const float st = s[t];
            const float inv_m = 1.f / (float)(Lg - 1), inv_Gm = 1.f / ((float)G * (float)(Lg - 1));
            float sp = 0.f, sg = 0.f;
            for (int n = lane; n < Lg; n += 64) {
                if (n == t) continue;
                const float x = s[n] - st, e = expf(-fabsf(x));
                sp += fmaxf(x, 0.f) + log1pf(e);
                sg += (x >= 0.f ? 1.f : e) / (1.f + e);
            }
            sp = ll_wave_sum(sp);
            sg = ll_wave_sum(sg);
            term = sp * inv_m;                           // NaN exactly when a score of the list is: x != x fails x >= 0, so sg is NaN too
            for (int n = lane; n < Lg; n += 64) {
                const float x = s[n] - st, e = expf(-fabsf(x));
                const float v = n == t ? -sg * inv_Gm : (x >= 0.f ? 1.f : e) / (1.f + e) * inv_Gm;
                d[n] = term != term ? term : v;          // a NaN score makes the whole row NaN, as the softmax does by itself
            }
        } else {
            float mx = -INFINITY;
            for (int n = lane; n < Lg; n += 64) mx = fmaxf(mx, s[n]);        // fmaxf drops a NaN: it comes back through the sum
            mx = ll_wave_max(mx);
            float se = 0.f;
            for (int n = lane; n < Lg; n += 64) se += expf(s[n] - mx);
            se = ll_wave_sum(se);
            term = logf(se) + mx - s[t];
            const float inv_G = 1.f / (float)G;
            for (int n = lane; n < Lg; n += 64) d[n] = (expf(s[n] - mx) / se - (n == t ? 1.f : 0.f)) * inv_G;
        }
        if (lane == 0) terms[g] = term;
    }
    if (lane == 0) red[wave] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        double p = 0.0;
        for (int w = 0; w < LL_WAVES; ++w) p += (double)red[w];
        part[blockIdx.x] = p;
    }
}

// The logQ-corrected softmax (include/cffm_hip.h): the softmax above on z_n = s_n - c_n, c_n = corr[i_n][0] - corr[i_t][1] for n != t and
// c_t = 0, i_n = lists[g][n] an index into the table corr [U][2].  The same layout - one wavefront per list, the same order of every sum -
// so an all-zero table gives the bits of list_loss_kernel<CFFM_LIST_SOFTMAX>: s - (0 - 0) is s, and a lane past the list adds what the
// strided loops above never formed (-inf to the maximum, an exact zero to the sum).  Every loop runs ceil(Lg / 64) trips on every lane
// and every branch is on a wave-uniform value; a lane past the end of the list loads the list's last element and its result is dropped
// by a select (a store is predicated).  The first stride's z stays in a register over the three passes: a list of at most 64 gathers
// its corrections once.
__device__ __forceinline__ float ll_logq_z(const float* __restrict__ s, const int32_t* __restrict__ ix, const float2* __restrict__ corr,
                                           int n, int t, float ct) {
    const float2 cv = corr[ix[n]];                       // one 8-byte load; column 1 is used for the target alone
    return s[n] - (n == t ? 0.f : cv.x - ct);
}

__global__ __launch_bounds__(64 * LL_WAVES) void list_loss_logq_kernel(const float* __restrict__ scores, int G, int Lg,
                                                                       const int32_t* __restrict__ target,
                                                                       const int32_t* __restrict__ lists,
                                                                       const float2* __restrict__ corr, int U, float* __restrict__ dout,
                                                                       float* __restrict__ terms, double* __restrict__ part) {
    __shared__ float red[LL_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * LL_WAVES + wave;
    float term = 0.f;                                    // a wavefront past the last list adds an exact zero to its workgroup's partial
    if (g < G) {                                         // wave-uniform
        const float* s = scores + (int64_t)g * Lg;
        const int32_t* ix = lists + (int64_t)g * Lg;
        float* d = dout + (int64_t)g * Lg;
        const int t = __builtin_amdgcn_readfirstlane(target[g]);
        bool ok = t >= 0 && t < Lg;
        if (ok) {                                        // every index of the list, before the first gather
            int bad = 0;
            for (int b = 0; b < Lg; b += 64) {
                const int i = ix[min(b + lane, Lg - 1)];
                bad |= (i < 0 || i >= U) ? 1 : 0;
            }
            ok = __ballot(bad) == 0ull;
        }
        if (!ok) {                                       // defined: a zero row and a zero term, neither s nor corr is read
            for (int b = 0; b < Lg; b += 64)
                if (b + lane < Lg) d[b + lane] = 0.f;
        } else {
            const float ct = corr[ix[t]].y;              // wave-uniform
            const float z0 = ll_logq_z(s, ix, corr, min(lane, Lg - 1), t, ct);
            float mx = lane < Lg ? z0 : -INFINITY;       // fmaxf drops a NaN: it comes back through the sum
            for (int b = 64; b < Lg; b += 64) {
                const float z = ll_logq_z(s, ix, corr, min(b + lane, Lg - 1), t, ct);
                mx = fmaxf(mx, b + lane < Lg ? z : -INFINITY);
            }
            mx = ll_wave_max(mx);
            float se = lane < Lg ? expf(z0 - mx) : 0.f;
            for (int b = 64; b < Lg; b += 64) {
                const float z = ll_logq_z(s, ix, corr, min(b + lane, Lg - 1), t, ct);
                se += b + lane < Lg ? expf(z - mx) : 0.f;
            }
            se = ll_wave_sum(se);
            term = logf(se) + mx - s[t];                 // z_t = s_t: the positive takes no correction
            const float inv_G = 1.f / (float)G;
            if (lane < Lg) d[lane] = (expf(z0 - mx) / se - (lane == t ? 1.f : 0.f)) * inv_G;
            for (int b = 64; b < Lg; b += 64) {
                const int n = b + lane;
                const float z = ll_logq_z(s, ix, corr, min(n, Lg - 1), t, ct);
                if (n < Lg) d[n] = (expf(z - mx) / se - (n == t ? 1.f : 0.f)) * inv_G;
            }
        }
        if (lane == 0) terms[g] = term;
    }
    if (lane == 0) red[wave] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        double p = 0.0;
        for (int w = 0; w < LL_WAVES; ++w) p += (double)red[w];
        part[blockIdx.x] = p;
    }
}

// second stage: the n workgroup partials, strided over 1024 threads in index order, lanes by the xor butterfly, waves in wave order
__global__ __launch_bounds__(1024) void list_loss_final_kernel(const double* __restrict__ part, int n, int G, float* __restrict__ loss) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) s += part[i];
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < 16; ++w) tot += red[w];
        loss[0] = (float)(tot / (double)G);
    }
}

static inline int64_t list_loss_blocks(int32_t G) { return ((int64_t)G + LL_WAVES - 1) / LL_WAVES; }

extern "C" int64_t cffm_list_loss_scratch_bytes(int32_t G) {
    if (G < 0) return -1;
    return (list_loss_blocks(G) + 1) * (int64_t)sizeof(double);          // never 0: an empty allocation has no address to hand in
}

extern "C" int cffm_list_loss(int32_t kind, const float* scores, int32_t G, int32_t Lg, const int32_t* target, float* dout,
                              float* terms, float* loss, void* scratch, void* stream) {
    if (kind != CFFM_LIST_BPR && kind != CFFM_LIST_SOFTMAX) return CFFM_ERR_BAD_SHAPE;
    if (G < 0 || Lg < 2 || (int64_t)G * Lg >= (1ll << 31)) return CFFM_ERR_BAD_SHAPE;
    if (G == 0) return 0;
    if (!scores || !target || !dout || !terms || !loss || !scratch) return CFFM_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)list_loss_blocks(G);
    if (kind == CFFM_LIST_BPR)
        hipLaunchKernelGGL(list_loss_kernel<CFFM_LIST_BPR>, dim3(nb), dim3(64 * LL_WAVES), 0, st, scores, G, Lg, target, dout, terms,
                           (double*)scratch);
    else
        hipLaunchKernelGGL(list_loss_kernel<CFFM_LIST_SOFTMAX>, dim3(nb), dim3(64 * LL_WAVES), 0, st, scores, G, Lg, target, dout, terms,
                           (double*)scratch);
    CFFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(list_loss_final_kernel, dim3(1), dim3(1024), 0, st, (const double*)scratch, nb, G, loss);
    CFFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cffm_list_loss_logq(int32_t kind, const float* scores, int32_t G, int32_t Lg, const int32_t* target, const int32_t* lists,
                                   const float* corr, int32_t U, float* dout, float* terms, float* loss, void* scratch, void* stream) {
    if (kind != CFFM_LIST_BPR && kind != CFFM_LIST_SOFTMAX) return CFFM_ERR_BAD_SHAPE;
    if (kind == CFFM_LIST_BPR) return CFFM_ERR_UNSUPPORTED;              // no agreed correction of the pairwise loss
    if (G < 0 || Lg < 2 || (int64_t)G * Lg >= (1ll << 31)) return CFFM_ERR_BAD_SHAPE;
    if (U < 1) return CFFM_ERR_BAD_SHAPE;
    if (G == 0) return 0;
    if (!scores || !target || !lists || !corr || !dout || !terms || !loss || !scratch) return CFFM_ERR_BAD_SHAPE;
    if ((uintptr_t)corr & 7) return CFFM_ERR_BAD_SHAPE;                  // a row of the table is one 8-byte load
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)list_loss_blocks(G);
    hipLaunchKernelGGL(list_loss_logq_kernel, dim3(nb), dim3(64 * LL_WAVES), 0, st, scores, G, Lg, target, lists, (const float2*)corr, U,
                       dout, terms, (double*)scratch);
    CFFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(list_loss_final_kernel, dim3(1), dim3(1024), 0, st, (const double*)scratch, nb, G, loss);
    CFFM_CHECK_LAUNCH();
    return 0;
}

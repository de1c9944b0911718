// Candidate ranking on the device: "for this context, which of these N items score highest?" and "where does the held-out item
// rank among all items?" (HR@k / NDCG@k).  The reference stops at RMSE / R2 (CFFM.py:583-615), so this replaces nothing in it; it
// is the sweep a trained recommender is used for, kept on the device like cffm_eval_sums: ids are expanded here, the scores come
// from cffm_predict, and a few numbers per context come back.
//
// ONE total order on the candidates of a context, shared by the three kernels and by tests/_rank_ref.py:
//   scores compare as IEEE floats with -0 == +0; NaN ranks below everything (-inf included); among equal scores the smaller
//   candidate position wins.
// As a 64-bit key, larger = better:  u = bits(score) with -0 taken as +0;  key32 = 0 for a NaN, ~u for a set sign bit, else
// u | 0x80000000;  key64 = key32 << 32 | (0xffffffff - position).  A skipped candidate has key64 = 0, which no real candidate can
// have (position < 2^31).  All compares are 64-bit integer compares, so every result is the same bits on every run.
//
// Top-k: a workgroup of 1024 threads takes one chunk of up to 8192 keys of one row into LDS, sorts blocks of L = pow2(max(k, 64)) keys
// (bitonic) and halves the number of blocks - larger key of a descending block and its ascending neighbour, then one bitonic merge -
// until the L best are left in descending order; it keeps the first k.  The k survivors of every chunk are the input of the next level (k <= 1024, so a level shrinks a row at least 8-fold) until one chunk
// per row is left, whose workgroup decodes the keys into idx / val / count.  One row with a million candidates is 128 workgroups in
// the first level; 4096 rows of 4082 candidates are one workgroup per row.  Every barrier sits in a loop whose trip count is a kernel
// argument (never under a per-lane condition).
#include "internal.hpp"
#include "rank_key.hpp"

#define RANK_CHUNK 8192
#define RANK_THREADS 1024
#define RANK_MAX_LEVELS 16
#define RANK_COUNT_THREADS 256

namespace {

// one step of a bitonic network over 2 * pairs keys in LDS: keys i and i + stride, larger first where (i & size) == 0
__device__ __forceinline__ void rank_cmpex(unsigned long long* lk, int tid, int pairs, int size, int stride) {
    for (int t = tid; t < pairs; t += RANK_THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const unsigned long long a = lk[i], b = lk[j];
        if ((a < b) == ((i & size) == 0)) { lk[i] = b; lk[j] = a; }
    }
}

// slot[f] = a where column f is fields[a] of a candidate tuple, -1 where the context keeps its id: by value, so the host list
// needs no device copy
struct FieldSlots { int8_t slot[CFFM_MAX_FIELDS]; };

__global__ __launch_bounds__(256) void expand_candidates_kernel(const int32_t* __restrict__ ctx, const int32_t* __restrict__ cand,
                                                                int64_t cand_ctx_stride, FieldSlots fs, int F, int nf, int N,
                                                                int64_t first, int64_t total, int32_t* __restrict__ ids_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / F;
    const int f = (int)(i - r * F);
    const int64_t g = first + r;
    const int64_t c = g / N;
    const int a = fs.slot[f];
    ids_out[i] = a >= 0 ? cand[c * cand_ctx_stride + (g - c * N) * nf + a] : ctx[c * F + f];
}

// One chunk of one row: FROM_SCORES builds the keys of candidates [chunk * 8192, ...) from the scores and the skip mask, otherwise
// the keys are the survivors of the level before (src [C][n_in]).  S keys (a power of two, L <= S <= 8192, >= the elements of a chunk;
// the tail beyond the row is key 0) are reduced to their L best in descending order, L = the power of two >= max(k, 64): only k
// of them are wanted, so nothing longer than L is ever sorted.  final == 0: the first k keys go to dst [C][chunks][k]; final != 0
// (chunks == 1): they are decoded into idx / val / count.
template <bool FROM_SCORES>
__global__ __launch_bounds__(RANK_THREADS) void topk_stage_kernel(const unsigned* __restrict__ sbits, int64_t row_stride,
                                                                  const uint8_t* __restrict__ skip, int64_t skip_stride,
                                                                  const unsigned long long* __restrict__ src, int64_t n_in, int chunks,
                                                                  int S, int L, int k, unsigned long long* __restrict__ dst, int final,
                                                                  int32_t* __restrict__ idx_out, unsigned* __restrict__ val_out,
                                                                  int32_t* __restrict__ count_out) {
    extern __shared__ unsigned long long lk[];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x / chunks;
    const int ch = (int)((int64_t)blockIdx.x - c * chunks);
    const int64_t e0 = (int64_t)ch * RANK_CHUNK;
    for (int i = tid; i < S; i += RANK_THREADS) {
        const int64_t e = e0 + i;
        unsigned long long key = 0;
        if (e < n_in) {
            if (FROM_SCORES) {
                if (!(skip && skip[c * skip_stride + e])) key = rank_key64(sbits[c * row_stride + e], (unsigned)e);
            } else {
                key = src[c * n_in + e];
            }
        }
        lk[i] = key;
    }
    __syncthreads();
    // blocks of L keys, sorted in alternating directions (even blocks descending)
    for (int size = 2; size <= L; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            rank_cmpex(lk, tid, S >> 1, size, stride);
            __syncthreads();
        }
    }
    // halve until one block is left: of a descending block and its ascending neighbour the element-wise larger keys are the best L of
    // their 2 L, as a bitonic sequence, which one bitonic merge sorts - again in alternating directions.  The survivors move to the
    // front (read, barrier, write: a pair's output overlaps the input of other pairs).
    const int lsh = 31 - __clz(L);
    for (int n = S; n > L; n >>= 1) {
        const int half = n >> 1;
        unsigned long long r[RANK_CHUNK / 2 / RANK_THREADS];
#pragma unroll
        for (int q = 0; q < RANK_CHUNK / 2 / RANK_THREADS; ++q) {
            const int t = tid + q * RANK_THREADS;
            r[q] = 0;
            if (t < half) {
                const int at = ((t >> lsh) << (lsh + 1)) + (t & (L - 1));
                const unsigned long long a = lk[at], b = lk[at + L];
                r[q] = a > b ? a : b;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RANK_CHUNK / 2 / RANK_THREADS; ++q) {
            const int t = tid + q * RANK_THREADS;
            if (t < half) lk[t] = r[q];
        }
        __syncthreads();
        for (int stride = L >> 1; stride > 0; stride >>= 1) {
            rank_cmpex(lk, tid, half >> 1, L, stride);
            __syncthreads();
        }
    }
    if (tid < k) {
        const unsigned long long key = tid < S ? lk[tid] : 0ull;
        if (!final) {
            dst[((int64_t)c * chunks + ch) * k + tid] = key;
        } else {
            const int64_t o = c * k + tid;
            if (key) {
                const unsigned pos = 0xffffffffu - (unsigned)key;
                idx_out[o] = (int32_t)pos;
                val_out[o] = sbits[c * row_stride + pos];                        // the score's own bits (-0, NaN payloads)
                const int lim = k < S ? k : S;
                const unsigned long long next = tid + 1 < lim ? lk[tid + 1] : 0ull;
                if (!next) count_out[c] = tid + 1;                               // the last real candidate of the sorted prefix
            } else {
                idx_out[o] = -1;
                val_out[o] = 0x7fc00000u;
                if (tid == 0) count_out[c] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(256) void rank_init_kernel(const int32_t* __restrict__ target, int C, int N, int32_t* __restrict__ rank_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C) return;
    const int t = target[i];
    rank_out[i] = (t >= 0 && t < N) ? 0 : -1;
}

// rank_out[c] += candidates of chunk `ch` of row c that beat the target (an integer count: the order of the adds does not matter)
__global__ __launch_bounds__(RANK_COUNT_THREADS) void rank_count_kernel(const unsigned* __restrict__ sbits, int64_t row_stride,
                                                                        const uint8_t* __restrict__ skip, int64_t skip_stride, int N,
                                                                        int chunks, const int32_t* __restrict__ target,
                                                                        int32_t* __restrict__ rank_out) {
    __shared__ int red[RANK_COUNT_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x / chunks;
    const int ch = (int)((int64_t)blockIdx.x - c * chunks);
    const int t = target[c];
    const bool valid = t >= 0 && t < N;
    // an invalid target is beaten by nobody: its row keeps the -1 of rank_init_kernel
    const unsigned long long tkey = valid ? rank_key64(sbits[c * row_stride + t], (unsigned)t) : ~0ull;
    const int64_t e0 = (int64_t)ch * RANK_CHUNK;
    const int64_t e1 = e0 + RANK_CHUNK < N ? e0 + RANK_CHUNK : N;
    int cnt = 0;
    for (int64_t e = e0 + tid; e < e1; e += RANK_COUNT_THREADS) {
        if (skip && skip[c * skip_stride + e]) continue;
        cnt += rank_key64(sbits[c * row_stride + e], (unsigned)e) > tkey ? 1 : 0;
    }
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if ((tid & 63) == 0) red[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < RANK_COUNT_THREADS / 64; ++w) tot += red[w];
        if (tot) atomicAdd(&rank_out[c], tot);
    }
}

struct TopkPlan {
    int levels;
    int64_t n_in[RANK_MAX_LEVELS];      // keys (level 0: candidates) per row entering level l
    int64_t chunks[RANK_MAX_LEVELS];    // workgroups per row of level l; the last level has one
    int64_t off[2], total;              // the two survivor buffers (levels write them alternately), bytes
};

inline int pow2_ceil(int64_t v) { int p = 1; while (p < v) p <<= 1; return p; }

inline int topk_plan(int64_t C, int64_t N, int64_t k, TopkPlan* p) {
    int64_t n = N;
    int l = 0;
    for (;; ++l) {
        if (l >= RANK_MAX_LEVELS) return CFFM_ERR_BAD_SHAPE;
        p->n_in[l] = n;
        p->chunks[l] = (n + RANK_CHUNK - 1) / RANK_CHUNK;
        if (p->chunks[l] == 1) break;
        n = p->chunks[l] * k;             // <= n / 8 + 1024 < n for n > 8192
    }
    p->levels = l + 1;
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    // level l writes buffer l & 1; the largest writers are levels 0 and 1
    const int64_t a = p->levels > 1 ? C * p->chunks[0] * k * 8 : 0;
    const int64_t b = p->levels > 2 ? C * p->chunks[1] * k * 8 : 0;
    p->off[0] = 256;
    p->off[1] = 256 + up(a);
    p->total = 256 + up(a) + up(b);
    return 0;
}

}  // namespace

extern "C" int cffm_expand_candidates_ex(const cffm_shape_t* s, const int32_t* ctx, int32_t C, const int32_t* fields, int32_t nf,
                                         const int32_t* cand, int64_t cand_ctx_stride, int32_t N, int64_t first, int32_t rows,
                                         int32_t* ids_out, void* stream) {
    int rc = check_shape(s);
    if (rc) return rc;
    if (nf < 1 || nf > s->F || !fields) return CFFM_ERR_BAD_SHAPE;
    FieldSlots fs;
    for (int f = 0; f < CFFM_MAX_FIELDS; ++f) fs.slot[f] = -1;
    for (int a = 0; a < nf; ++a) {
        const int f = fields[a];
        if (f < 0 || f >= s->F || fs.slot[f] >= 0) return CFFM_ERR_BAD_SHAPE;      // outside [0, F), or the same field twice
        fs.slot[f] = (int8_t)a;
    }
    if (N < 1 || C < 0 || first < 0 || rows < 0) return CFFM_ERR_BAD_SHAPE;
    if (first + (int64_t)rows > (int64_t)C * N) return CFFM_ERR_BAD_SHAPE;
    if (cand_ctx_stride < 0 || (cand_ctx_stride != 0 && cand_ctx_stride < (int64_t)N * nf)) return CFFM_ERR_BAD_SHAPE;
    if (C == 0 || rows == 0) return 0;
    if (!ctx || !cand || !ids_out) return CFFM_ERR_BAD_SHAPE;
    const int64_t total = (int64_t)rows * s->F;
    hipLaunchKernelGGL(expand_candidates_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctx, cand,
                       cand_ctx_stride, fs, (int)s->F, (int)nf, (int)N, first, total, ids_out);
    CFFM_CHECK_LAUNCH();
    return 0;
}

// one field, one list for every context: the same kernel
extern "C" int cffm_expand_candidates(const cffm_shape_t* s, const int32_t* ctx, int32_t C, int32_t field, const int32_t* cand, int32_t N,
                                      int64_t first, int32_t rows, int32_t* ids_out, void* stream) {
    return cffm_expand_candidates_ex(s, ctx, C, &field, 1, cand, 0, N, first, rows, ids_out, stream);
}

extern "C" int64_t cffm_topk_scratch_bytes(int32_t C, int32_t N, int32_t k) {
    if (C < 0 || N < 1 || k < 1 || k > 1024) return -1;
    TopkPlan p;
    if (topk_plan(C, N, k, &p)) return -1;
    return p.total;
}

extern "C" int cffm_topk(const float* scores, int64_t row_stride, const uint8_t* skip, int64_t skip_stride, int32_t C, int32_t N, int32_t k,
                         void* scratch, int32_t* idx_out, float* val_out, int32_t* count_out, void* stream) {
    if (C < 0 || N < 1 || k < 1 || k > 1024 || row_stride < N || (skip && skip_stride < N)) return CFFM_ERR_BAD_SHAPE;
    TopkPlan p;
    if (topk_plan(C, N, k, &p)) return CFFM_ERR_BAD_SHAPE;
    if ((int64_t)C * p.chunks[0] >= (1ll << 31)) return CFFM_ERR_BAD_SHAPE;      // workgroups of the first level
    if (C == 0) return 0;
    if (!scores || !scratch || !idx_out || !val_out || !count_out) return CFFM_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const unsigned* sbits = (const unsigned*)scores;
    unsigned long long* buf[2] = {(unsigned long long*)((char*)scratch + p.off[0]), (unsigned long long*)((char*)scratch + p.off[1])};
    const int L = pow2_ceil(k) < 64 ? 64 : pow2_ceil(k);
    for (int l = 0; l < p.levels; ++l) {
        const int final = l == p.levels - 1;
        const int chunks = (int)p.chunks[l];
        const int S = chunks > 1 ? RANK_CHUNK : (pow2_ceil(p.n_in[l]) < L ? L : pow2_ceil(p.n_in[l]));
        const dim3 grid((unsigned)((int64_t)C * chunks));
        const unsigned long long* src = l ? buf[(l - 1) & 1] : nullptr;
        unsigned long long* dst = final ? nullptr : buf[l & 1];
        if (l == 0)
            hipLaunchKernelGGL(topk_stage_kernel<true>, grid, dim3(RANK_THREADS), (size_t)S * 8, st, sbits, row_stride, skip, skip_stride, src,
                               p.n_in[l], chunks, S, L, (int)k, dst, final, idx_out, (unsigned*)val_out, count_out);
        else
            hipLaunchKernelGGL(topk_stage_kernel<false>, grid, dim3(RANK_THREADS), (size_t)S * 8, st, sbits, row_stride, skip, skip_stride, src,
                               p.n_in[l], chunks, S, L, (int)k, dst, final, idx_out, (unsigned*)val_out, count_out);
        CFFM_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int cffm_rank_of(const float* scores, int64_t row_stride, const uint8_t* skip, int64_t skip_stride, int32_t C, int32_t N,
                            const int32_t* target, int32_t* rank_out, void* stream) {
    if (C < 0 || N < 1 || row_stride < N || (skip && skip_stride < N)) return CFFM_ERR_BAD_SHAPE;
    const int chunks = (N + RANK_CHUNK - 1) / RANK_CHUNK;
    if ((int64_t)C * chunks >= (1ll << 31)) return CFFM_ERR_BAD_SHAPE;
    if (C == 0) return 0;
    if (!scores || !target || !rank_out) return CFFM_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rank_init_kernel, dim3((unsigned)(((int64_t)C + 255) / 256)), dim3(256), 0, st, target, (int)C, (int)N, rank_out);
    CFFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)((int64_t)C * chunks)), dim3(RANK_COUNT_THREADS), 0, st, (const unsigned*)scores,
                       row_stride, skip, skip_stride, (int)N, chunks, target, rank_out);
    CFFM_CHECK_LAUNCH();
    return 0;
}

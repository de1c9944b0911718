// Optimiser step: tf.train.AdagradOptimizer(lr, initial_accumulator_value=1e-8).minimize (CFFM.py:523-524).
//
//   reduce_slabs    sum of the CFFM_NSLAB split-K partial gradients in slab order (bitwise reproducible)
//   dense_adagrad   acc += g*g; v -= lr*g/sqrt(acc)                        (no epsilon, TF semantics)
//   sparse_adagrad  IndexedSlices semantics: duplicate ids are summed FIRST, then one update per distinct
//                   row; rows not in the batch and their accumulators are untouched.  Implemented as a
//                   stable radix sort of (id, slot) followed by one wavefront per segment head that walks
//                   its segment in slot order - HBM-bound: per distinct row 5 x (K+D+1) x 4 bytes.
#include "internal.hpp"

#include <cmath>
#include <cstring>
#include <type_traits>
#include <rocprim/device/device_radix_sort.hpp>

// One workgroup = 64 groups of four consecutive gradients (every member of theta and every slab range is 16-byte aligned,
// cffm_theta_layout) x 4 wavefronts, each adding a quarter of the range's slabs with 16-byte loads; the four partial sums
// meet in LDS and are added in wavefront order.  Bitwise reproducible, and four times the bytes in flight of the
// one-thread-per-gradient loop it replaces (that one kept 16 x 4-byte loads per lane in flight on 161 workgroups and
// reached 3 TB/s on the 26 MB of slabs of the frappe step: update_all 11.4 us; this form 9.8 us; an 8-way split over
// half-wavefronts, twice the workgroups, was slower again at 10.8 us).  That form asked for its slabs in batches of 8 loads, each
// batch ending in vmcnt(0) before the next one was issued, behind two dependent vector loads of the dynamically indexed plan entry:
// about ten serialized round trips.  Now the plan is read with scalar loads and selected with compares, and a quarter's slabs go
// through a ring of REDUCE_RING loads that never drains (profiles/update_chains.md); the add order is what it was.
#define REDUCE_GROUPS 64
#define REDUCE_RING 16
// The load that follows may not be moved in front of the add that precedes it (an empty statement that the compiler must assume
// reads the sum and memory): without it the optimizer gathers the adds of a ring in front of its loads and the ring drains.
#define REDUCE_PIN(s) asm volatile("" : "+v"((s).x), "+v"((s).y), "+v"((s).z), "+v"((s).w) : : "memory")
static inline int reduce_slab_wgs(int64_t n) { return (int)((n / 4 + REDUCE_GROUPS - 1) / REDUCE_GROUPS); }
__device__ __forceinline__ void reduce_slabs_body(int bid, const float* __restrict__ gpart, int64_t n, const SlabPlan& sp,
                                                  float* __restrict__ grad, float* __restrict__ theta,
                                                  float* __restrict__ acc, float lr) {
    __shared__ float4 part[4][REDUCE_GROUPS];
    const int g = threadIdx.x & 63, q = threadIdx.x >> 6;          // group, quarter
    const int64_t i = ((int64_t)bid * REDUCE_GROUPS + g) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) {
        // the range of i: every entry of the plan is read at a constant index of the argument (scalar loads) and selected with a
        // compare - a dynamically indexed by-value argument costs two dependent vector loads before the first slab byte is asked for
        int64_t rel = sp.r[0].base - sp.r[0].off, len = sp.r[0].len;      // slab 0 of gradient i is gpart[rel + i]
        int nslab = sp.r[0].nslab;
#pragma unroll
        for (int r = 1; r < CFFM_MAX_LAYERS + 3; ++r) {
            const bool hit = r < sp.n && i >= sp.r[r].off;
            rel = hit ? sp.r[r].base - sp.r[r].off : rel; len = hit ? sp.r[r].len : len; nslab = hit ? sp.r[r].nslab : nslab;
        }
        const int64_t stride = len / 4;
        const int per = (nslab + 3) / 4, k0 = q * per, k1 = min(nslab, k0 + per);
        if (k0 < k1) {
            // A ring of REDUCE_RING loads: slab k is added and slab k + REDUCE_RING asked for in its place, so REDUCE_RING - 1 or
            // REDUCE_RING 16-byte loads per lane are in flight from the first add to the last full ring.  p walks the slabs by the
            // stride and stops at slab k1 - 1 (a load past the quarter re-reads that slab and is not added).  Add order: k ascending.
            const float4* p = reinterpret_cast<const float4*>(gpart + rel + i) + (int64_t)k0 * stride;
            float4 v[REDUCE_RING];
#pragma unroll
            for (int j = 0; j < REDUCE_RING; ++j) {
                v[j] = *p;
                p += k0 + j + 1 < k1 ? stride : 0;
            }
            int k = k0;
            for (; k + 2 * REDUCE_RING <= k1; k += REDUCE_RING) {       // every slab of the next ring exists
#pragma unroll
                for (int j = 0; j < REDUCE_RING; ++j) {
                    s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w;
                    REDUCE_PIN(s);
                    v[j] = *p;
                    p += stride;
                }
            }
            if (k + REDUCE_RING < k1) {                                  // a last, partial ring (p is at slab k + REDUCE_RING here)
#pragma unroll
                for (int j = 0; j < REDUCE_RING; ++j) {
                    s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w;
                    REDUCE_PIN(s);
                    v[j] = *p;
                    p += k + REDUCE_RING + j + 1 < k1 ? stride : 0;
                }
                k += REDUCE_RING;
            }
#pragma unroll
            for (int j = 0; j < REDUCE_RING; ++j) {
                if (k + j < k1) { s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w; }
            }
        }
    }
    part[q][g] = s;
    __syncthreads();
    if (q != 0 || i >= n) return;
#pragma unroll
    for (int e = 1; e < 4; ++e) {
        const float4 p = part[e][g];
        s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
    *reinterpret_cast<float4*>(grad + i) = s;
    if (theta != nullptr) {                 // fused dense Adagrad (single-GPU step)
        float4 a = *reinterpret_cast<float4*>(acc + i), t = *reinterpret_cast<float4*>(theta + i);
        a.x += s.x * s.x; a.y += s.y * s.y; a.z += s.z * s.z; a.w += s.w * s.w;
        t.x -= lr * s.x / sqrtf(a.x); t.y -= lr * s.y / sqrtf(a.y); t.z -= lr * s.z / sqrtf(a.z); t.w -= lr * s.w / sqrtf(a.w);
        *reinterpret_cast<float4*>(acc + i) = a;
        *reinterpret_cast<float4*>(theta + i) = t;
    }
}

__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ gpart, int64_t n, SlabPlan sp,
                                                           float* __restrict__ grad, float* __restrict__ theta,
                                                           float* __restrict__ acc, float lr) {
    reduce_slabs_body(blockIdx.x, gpart, n, sp, grad, theta, acc, lr);
}

// Late loss normalisation of the data-parallel step: the backward pass ran with dL/dout = (out - y) / Bg, i.e.
// WITHOUT the 1/L of the RMSE-style loss (CFFM.py:493), because L needs the loss-term sum over the GLOBAL batch,
// which only exists after the all-reduce that also carries the gradients.  Every gradient is linear in dL/dout,
// so the factor 1/L = rsqrt(sum / Bg + 1e-10) is applied here, on the summed gradient.
__device__ __forceinline__ float late_scale(const LateScale& ls) {
    return ls.on ? 1.f / sqrtf(ls.sum[0] * ls.inv_Bg + 1e-10f) : 1.f;
}

// ---- the update rules: rule(w, s1, s2, g) moves one weight (in memory) and its slots by the gradient g ---------------------
// A rule is a template parameter of every body and kernel below, so the Adagrad instantiations carry no branch on the optimizer.
// slot(): the rule reads s1 (a NULL slot pointer is never formed from a table the caller did not pass).
struct AdagradRule {
    float lr;
    __device__ __forceinline__ bool slot() const { return true; }
    __device__ __forceinline__ void operator()(float& w, float* s1, float*, float g) const {
        const float a = *s1 + g * g;
        *s1 = a;
        w -= lr * g / sqrtf(a);
    }
};

// the other optimizers of CFFM.py:519-529 (TF-1.14 semantics), switched at run time on OptConst::opt
struct OptConst { int opt; float lr, lr_t, b1, b2, omb1, omb2, eps, mom; };   // omb* = 1 - beta, rounded once from double

__device__ __forceinline__ void opt_update(float& w, float* s1, float* s2, float g, const OptConst& c) {
    if (c.opt == CFFM_OPT_SGD) {
        w -= c.lr * g;
    } else if (c.opt == CFFM_OPT_MOMENTUM) {
        const float a = c.mom * (*s1) + g;
        *s1 = a;
        w -= c.lr * a;
    } else {                                      // Adam
        const float m = c.b1 * (*s1) + c.omb1 * g;
        const float v = c.b2 * (*s2) + c.omb2 * g * g;
        *s1 = m; *s2 = v;
        w -= c.lr_t * m / (sqrtf(v) + c.eps);
    }
}

struct OptRule {
    OptConst c;
    __device__ __forceinline__ bool slot() const { return c.opt == CFFM_OPT_MOMENTUM; }    // (Adam only runs in dense_opt_kernel)
    __device__ __forceinline__ void operator()(float& w, float* s1, float* s2, float g) const {
        float wv = w;                             // the weight is read before the slots are written
        opt_update(wv, s1, s2, g, c);
        w = wv;
    }
};

// the constants of CFFM.py:519-529, for the single-GPU step and the multi-GPU apply alike (step >= 1; only Adam reads lr_t)
static OptRule opt_rule(const cffm_shape_t* s, int64_t step) {
    OptConst c;
    c.opt = s->optimizer; c.lr = s->lr; c.b1 = 0.9f; c.b2 = 0.999f; c.omb1 = (float)(1.0 - 0.9); c.omb2 = (float)(1.0 - 0.999); c.eps = 1e-8f; c.mom = 0.95f;
    c.lr_t = (float)((double)s->lr * sqrt(1.0 - pow(0.999, (double)step)) / (1.0 - pow(0.9, (double)step)));
    return OptRule{c};
}

// dense rule on theta with the late 1/L; thread 0 also writes the loss of the global batch
template <class Rule>
__device__ __forceinline__ void dense_late_body(int bid, float* __restrict__ v, float* __restrict__ s1, const float* __restrict__ grad,
                                                int64_t n, const Rule& rule, const LateScale& ls, float* __restrict__ loss_out) {
    const int64_t i = (int64_t)bid * 256 + threadIdx.x;
    if (i == 0 && loss_out != nullptr) loss_out[0] = ls.on ? sqrtf(ls.sum[0] * ls.inv_Bg + 1e-10f) : ls.sum[0] * ls.inv_Bg;
    if (i >= n) return;
    const float g = grad[i] * late_scale(ls);
    rule(v[i], rule.slot() ? s1 + i : nullptr, nullptr, g);
}

template <class Rule>
__global__ __launch_bounds__(256) void dense_late_kernel(float* __restrict__ v, float* __restrict__ s1, const float* __restrict__ grad,
                                                         int64_t n, Rule rule, LateScale ls, float* __restrict__ loss_out) {
    dense_late_body(blockIdx.x, v, s1, grad, n, rule, ls, loss_out);
}

// Sorted order of n <= 8192 unique keys (id << 32 | slot) without a sort: the place of a key is the number of keys below
// it.  Workgroup w of nwg places keys [w*kpw, (w+1)*kpw): its 256 threads split the n candidates, count per key in
// registers, wave/block-reduce, and the first kpw threads store their key at its rank.  ids are read with a stride
// (the id column of the packed rows of the data-parallel step, or a plain id array with stride 1).
#define RANK_KPW_MAX 32
__device__ __forceinline__ void rank_place_body(int wg, int nwg, const int32_t* __restrict__ ids, int64_t id_stride, int n,
                                                unsigned long long* __restrict__ out, float* cnt /* LDS [4][RANK_KPW_MAX] */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kpw = (n + nwg - 1) / nwg, k0 = wg * kpw;
    unsigned long long mine[RANK_KPW_MAX];
#pragma unroll
    for (int k = 0; k < RANK_KPW_MAX; ++k) {
        const int slot = k0 + k;
        mine[k] = (k < kpw && slot < n) ? (((unsigned long long)(unsigned)ids[(int64_t)slot * id_stride] << 32) | (unsigned)slot) : 0ull;
    }
    int c[RANK_KPW_MAX];
#pragma unroll
    for (int k = 0; k < RANK_KPW_MAX; ++k) c[k] = 0;
    for (int j = tid; j < n; j += 256) {
        const unsigned long long kj = ((unsigned long long)(unsigned)ids[(int64_t)j * id_stride] << 32) | (unsigned)j;
#pragma unroll
        for (int k = 0; k < RANK_KPW_MAX; ++k)
            if (k < kpw) c[k] += kj < mine[k] ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < RANK_KPW_MAX; ++k) {
        if (k < kpw) {
            const float t = wave_sum((float)c[k]);               // counts <= 8192: exact in fp32
            if (lane == 0) cnt[wave * RANK_KPW_MAX + k] = t;
        }
    }
    __syncthreads();
    if (tid < kpw && k0 + tid < n) {
        const int rank = (int)(((cnt[tid] + cnt[RANK_KPW_MAX + tid]) + cnt[2 * RANK_KPW_MAX + tid]) + cnt[3 * RANK_KPW_MAX + tid]);
        const int slot = k0 + tid;
        out[rank] = ((unsigned long long)(unsigned)ids[(int64_t)slot * id_stride] << 32) | (unsigned)slot;
    }
}

// Global order of n_runs sorted runs of m keys each (every rank's own run, made by the single-launch forward) without
// sorting them again: the place of the key at (run r, position p) is p + sum over the other runs of the number of keys
// that precede it there - an upper bound on its id in the runs before r, a lower bound in the runs after r (the global
// slot r*m + local slot breaks id ties in run order).  Every workgroup stages all ids (4*n bytes) in LDS once and its
// 256 threads run n_runs - 1 binary searches each.
struct MergeArgs {
    const float* rows;            // n_runs blocks of [m*W | m keys (u64)]
    int64_t block_floats;         // m * (W + 2)
    int64_t keys_off;             // m * W
    int m, n_runs;
    unsigned long long* out;      // [n_runs * m] keys (id << 32 | global slot) in global order
};
__device__ __forceinline__ void merge_runs_body(int wg, const MergeArgs& a, unsigned* ids_l /* LDS [n] */) {
    const int n = a.m * a.n_runs;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int r = e / a.m, p = e - r * a.m;
        const unsigned long long k = reinterpret_cast<const unsigned long long*>(a.rows + (int64_t)r * a.block_floats + a.keys_off)[p];
        ids_l[e] = (unsigned)(k >> 32);
    }
    __syncthreads();
    const int e = wg * 256 + threadIdx.x;
    if (e >= n) return;
    const int r = e / a.m, p = e - r * a.m;
    const unsigned long long k = reinterpret_cast<const unsigned long long*>(a.rows + (int64_t)r * a.block_floats + a.keys_off)[p];
    const unsigned id = (unsigned)(k >> 32);
    int rank = p;
    for (int q = 0; q < a.n_runs; ++q) {
        if (q == r) continue;
        const unsigned* run = ids_l + q * a.m;
        int lo = 0, hi = a.m;                                  // first position whose id is > id (q < r) or >= id (q > r)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const unsigned v = run[mid];
            const bool before = q < r ? v <= id : v < id;
            if (before) lo = mid + 1; else hi = mid;
        }
        rank += lo;
    }
    a.out[rank] = ((unsigned long long)id << 32) | (unsigned long long)(unsigned)(r * a.m + (int)(k & 0xffffffffull));
}

// first launch of the data-parallel apply, sorted runs: dense rule with the late 1/L ∥ merge of the per-rank runs
template <class Rule>
__global__ __launch_bounds__(256) void dp_head_merge_kernel(float* __restrict__ v, float* __restrict__ s1, const float* __restrict__ grad,
                                                            int64_t n, Rule rule, LateScale ls, float* __restrict__ loss_out,
                                                            int n_dense, MergeArgs ma) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if ((int)blockIdx.x < n_dense) dense_late_body(blockIdx.x, v, s1, grad, n, rule, ls, loss_out);
    else merge_runs_body(blockIdx.x - n_dense, ma, reinterpret_cast<unsigned*>(smem));
}

// first launch of the data-parallel apply, n_rows <= 8192 without runs: dense rule with the late 1/L ∥ placement of the gathered keys
template <class Rule>
__global__ __launch_bounds__(256) void dp_head_kernel(float* __restrict__ v, float* __restrict__ s1, const float* __restrict__ grad,
                                                      int64_t n, Rule rule, LateScale ls, float* __restrict__ loss_out, int n_dense,
                                                      const int32_t* __restrict__ ids, int64_t id_stride, int n_keys, int n_rank,
                                                      unsigned long long* __restrict__ keys_out) {
    __shared__ float cnt[4 * RANK_KPW_MAX];
    if ((int)blockIdx.x < n_dense) dense_late_body(blockIdx.x, v, s1, grad, n, rule, ls, loss_out);
    else rank_place_body(blockIdx.x - n_dense, n_rank, ids, id_stride, n_keys, keys_out, cnt);
}

// last launch of cffm_dp_local: slab reduction (no update) ∥ packing of (id | dEi | dEo | dfb) rows + the local loss sum
struct PackArgs {
    const int32_t* ids;
    int64_t n_slots;
    int K, D, B;
    const float *dEi, *dEo, *dfb, *sqerr;
    float *sum_dst, *rows, *scalars;
    const unsigned long long* keys_sorted;   // non-NULL: appended after the rows as this rank's sorted run
};
__device__ __forceinline__ void pack_rows_body(int bid, int nblk, const PackArgs& a, float* red) {
    const int W = 1 + a.K + a.D + 1;
    const int64_t total = a.n_slots * W;
    if (bid == 0) {                                  // loss-term sum of this rank, fixed order
        float part = 0.f;
        for (int i = threadIdx.x; i < a.B; i += 256) part += a.sqerr[i];
        const float sum = block_sum(part, red);
        if (threadIdx.x == 0) { a.sum_dst[0] = sum; a.scalars[0] = sum; }
    }
    for (int64_t i = (int64_t)bid * 256 + threadIdx.x; i < total; i += (int64_t)nblk * 256) {
        const int64_t slot = i / W;
        const int c = (int)(i - slot * W);
        float v;
        if (c == 0) v = __int_as_float(a.ids[slot]);
        else if (c <= a.K) v = a.dEi ? a.dEi[slot * a.K + (c - 1)] : 0.f;           // disabled branch: its columns travel as zeros
        else if (c <= a.K + a.D) v = a.dEo ? a.dEo[slot * a.D + (c - 1 - a.K)] : 0.f;
        else v = a.dfb[slot];
        a.rows[i] = v;
    }
    if (a.keys_sorted != nullptr) {
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.rows + total);      // total * 4 bytes is 8-byte aligned: see cffm_dp_tail
        for (int64_t i = (int64_t)bid * 256 + threadIdx.x; i < a.n_slots; i += (int64_t)nblk * 256) dst[i] = a.keys_sorted[i];
    }
}
__global__ __launch_bounds__(256) void dp_tail_kernel(const float* __restrict__ gpart, int64_t n, SlabPlan sp, float* __restrict__ grad,
                                                      int n_reduce, PackArgs pa, int n_pack) {
    __shared__ float red[4];
    if ((int)blockIdx.x < n_reduce) reduce_slabs_body(blockIdx.x, gpart, n, sp, grad, nullptr, nullptr, 0.f);
    else pack_rows_body(blockIdx.x - n_reduce, n_pack, pa, red);
}

int cffm_dp_tail(const StepCtx& c, const int32_t* ids, float* grad, float* rows, bool with_run, hipStream_t st) {
    const cffm_shape_t* s = c.s;
    const cffm_theta_layout_t& tl = c.tl;
    const cffm_ws_layout_t& wl = c.wl;
    const RowGrads r = RowGrads::of_ws(c);
    PackArgs pa;
    pa.ids = ids; pa.n_slots = (int64_t)c.B * s->F; pa.K = s->K; pa.D = s->D; pa.B = c.B;
    pa.dEi = r.dEi; pa.dEo = r.dEo; pa.dfb = r.dfb;
    pa.sqerr = c.at<const float>(wl.sqerr); pa.sum_dst = grad + tl.n; pa.rows = rows; pa.scalars = c.at(wl.scalars);
    // n_slots * W floats: W = K + D + 2 is even for the float4-aligned K, D this library accepts, so the run is 8-byte aligned
    pa.keys_sorted = with_run ? c.at<const unsigned long long>(wl.sort_vals) : nullptr;
    const int n_reduce = reduce_slab_wgs(tl.n);
    const int64_t total = pa.n_slots * (1 + s->K + s->D + 1);
    int n_pack = (int)((total + 1023) / 1024);
    if (n_pack > 2048) n_pack = 2048;
    hipLaunchKernelGGL(dp_tail_kernel, dim3(n_reduce + n_pack), dim3(256), 0, st, c.at<const float>(wl.gpart), (int64_t)tl.n, c.sp,
                       grad, n_reduce, pa, n_pack);
    CFFM_CHECK_LAUNCH();
    return 0;
}

// An id outside [0, M) is keyed as M: the radix sorts look at ceil(log2(M + 1)) id bits only, and a raw bad id whose low
// bits equal a valid id would land inside that id's run and split its segment in two (two wavefronts updating one row).
// All bad ids form ONE segment with id M, which every update kernel skips (id >= M).
__global__ __launch_bounds__(256) void pack_keys_kernel(const int32_t* __restrict__ ids, unsigned long long* keys, int64_t n,
                                                        int64_t id_stride, int M) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int raw = ids[i * id_stride];
        keys[i] = ((unsigned long long)(unsigned)((raw < 0 || raw >= M) ? M : raw) << 32) | (unsigned long long)i;
    }
}

#include "sort_body.hpp"

__global__ __launch_bounds__(256) void small_sort_kernel(const unsigned long long* __restrict__ in,
                                                         unsigned long long* __restrict__ out, int n, int id_bits) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    small_sort_body(in, nullptr, out, n, id_bits, smem);
}

// ---- the segment walk ---------------------------------------------------------------------------------------------------------
// One wavefront per sorted position of the keys (id << 32 | slot); only segment heads work.  Each lane owns the columns lane,
// lane + 64, ... of the row (inner | outer | bias; a disabled branch, dEi / dEo == NULL, has none) and sums each over the duplicates
// of the id in slot order - ascending sorted position, one accumulator per column starting from 0.f: every "bitwise reproducible"
// of DESIGN.md rests on this order - then hands (id, table, column within the table) and the sum to the sink: sink.at() locates the
// element, under the walk's own column comparison so that the table is a constant there, and sink(at, sum) does the one thing
// that is done with it.  Ids outside [0, M) (keyed as M, see pack_keys_kernel) are skipped.  Slot s reads its gradients at s * sE* of RowGrads; run_len > 0: slot s lives in block
// s / run_len at local index s % run_len, and blocks are run_stride floats apart (the per-rank runs of the data-parallel apply).
struct SparseArgs {
    const unsigned long long* keys;
    int64_t n;
    int M, K, D;
    const float *dEi, *dEo, *dfb;
    int64_t sEi, sEo, sfb;
    int run_len;
    int64_t run_stride;
    float inv_run_len;
};
enum { T_INNER = 0, T_OUTER = 1, T_BIAS = 2 };
static const cffm_tables_t NO_TABLES = {nullptr, nullptr, nullptr};

//
// The walk of a head: its 64 lanes read the next 64 keys of the run in one load, a ballot gives the number that carry the id (a
// longer run goes on in chunks of 64), and slot j of the chunk is handed from lane j to all lanes (v_readlane) - no gradient load
// waits for a key load.  A lane carries NCH columns (lane, lane + 64, ...) through the same walk, the lone bias column of
// W = K + D + 1 = 65 included: a column past W - 1 reads column W - 1 again and is dropped at the end.  The sink's element (weight
// and slot) is asked for before the first gradient (sink.pre).  The gradients of 8 / 4 / 2 / 1 slots are asked for together and then
// added in slot order.
template <int NCH, class Sink>
__device__ __forceinline__ void segment_walk_cols(const SparseArgs& a, const Sink& sink, int64_t pos, unsigned long long kq, int id,
                                                  int c0, int W, int Ki, int lane) {      // kq: key pos + lane
    const unsigned long long* __restrict__ keys = a.keys;
    const int64_t n = a.n;
    const float* gp[NCH];              // column c of slot 0 of block 0
    int64_t gs[NCH];                   // floats from slot to slot
    typename Sink::At at[NCH];
    typename Sink::Pre pre[NCH];
    float g[NCH];
    bool live[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = c0 + ch * 64 + lane;
        live[ch] = c < W;
        const int cc = live[ch] ? c : W - 1;
        // each table is named by a constant where its pointer is read, and the lane's one is selected afterwards (a table number
        // that depends on the lane indexes the argument struct, which then lives in scratch memory)
        const bool in_i = cc < Ki, in_o = !in_i && cc < W - 1;
        const typename Sink::At ai = sink.at(id, T_INNER, in_i ? cc : 0), ao = sink.at(id, T_OUTER, in_o ? cc - Ki : 0),
                                ab = sink.at(id, T_BIAS, 0);
        gp[ch] = in_i ? a.dEi + cc : (in_o ? a.dEo + (cc - Ki) : a.dfb);
        gs[ch] = in_i ? a.sEi : (in_o ? a.sEo : a.sfb);
        at[ch] = in_i ? ai : (in_o ? ao : ab);
        pre[ch] = sink.pre(at[ch]);
        g[ch] = 0.f;
    }
    for (int64_t q0 = pos;; q0 += 64) {
        if (q0 != pos) kq = q0 + lane < n ? keys[q0 + lane] : ~0ull;  // (id -1: never the id of a head that works)
        const unsigned long long in_run = __ballot((int)(kq >> 32) == id);
        const int cnt = ~in_run == 0ull ? 64 : __builtin_ctzll(~in_run);     // the run is a prefix of the chunk (sorted keys)
        int sl = (int)(unsigned)(kq & 0xffffffffull), blk = 0;
        if (a.run_len > 0) {
            blk = fast_div(sl, a.inv_run_len);
            sl -= blk * a.run_len;
        }
        // slots j .. j + N - 1 of the chunk: N x NCH loads, then the adds in slot order
        auto slots = [&](int j, auto N) {
            float v[decltype(N)::value][NCH];
#pragma unroll
            for (int t = 0; t < decltype(N)::value; ++t) {
                const int64_t s = __builtin_amdgcn_readlane(sl, j + t);
                const int64_t boff = (int64_t)__builtin_amdgcn_readlane(blk, j + t) * a.run_stride;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) v[t][ch] = gp[ch][boff + s * gs[ch]];
            }
#pragma unroll
            for (int t = 0; t < decltype(N)::value; ++t)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) g[ch] += v[t][ch];
        };
        int j = 0;
        for (; j + 8 <= cnt; j += 8) slots(j, std::integral_constant<int, 8>());
        if (cnt & 4) { slots(j, std::integral_constant<int, 4>()); j += 4; }
        if (cnt & 2) { slots(j, std::integral_constant<int, 2>()); j += 2; }
        if (cnt & 1) slots(j, std::integral_constant<int, 1>());
        if (cnt < 64) break;
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
        if (live[ch]) sink(at[ch], pre[ch], g[ch]);
}

template <class Sink>
__device__ __forceinline__ void segment_walk(int bid, const SparseArgs& a, const Sink& sink) {
    const unsigned long long* __restrict__ keys = a.keys;
    const int64_t n = a.n;
    const int64_t pos = (int64_t)bid * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pos >= n) return;
    // the first 64 keys from pos on and the key in front of pos: one round trip
    const unsigned long long kq = pos + lane < n ? keys[pos + lane] : ~0ull;
    const int id_prev = (int)(keys[pos > 0 ? pos - 1 : 0] >> 32);
    const int id = __builtin_amdgcn_readfirstlane((int)(kq >> 32));
    if (pos > 0 && id_prev == id) return;                             // not a segment head
    if (id < 0 || id >= a.M) return;
    const int W = (a.dEi ? a.K : 0) + (a.dEo ? a.D : 0) + 1;
    const int Ki = a.dEi ? a.K : 0;
    if (W <= 64) segment_walk_cols<1>(a, sink, pos, kq, id, 0, W, Ki, lane);
    else if (W <= 128) segment_walk_cols<2>(a, sink, pos, kq, id, 0, W, Ki, lane);
    else
        for (int c0 = 0; c0 < W; c0 += 256) segment_walk_cols<4>(a, sink, pos, kq, id, c0, W, Ki, lane);
}

// the sinks: At at(id, table, col), Pre pre(at) - what of the element is read, asked for before the sum exists - and
// operator()(at, pre, sum).  Element (id, col) of table t of a [M][K] | [M][D] | [M] triple is table_of(T, t)[row_off(..)]:
__device__ __forceinline__ int64_t row_off(int K, int D, int id, int t, int col) {
    if (t == T_INNER) return (int64_t)id * K + col;
    if (t == T_OUTER) return (int64_t)id * D + col;
    return id;
}
__device__ __forceinline__ float* table_of(const cffm_tables_t& T, int t) {
    if (t == T_INNER) return T.inner_emb;
    if (t == T_OUTER) return T.outer_emb;
    return T.feat_bias;
}
// apply the rule to the row and its slot row (s.* is not read where the rule keeps no slot); LATE: the sum is first scaled by the late 1/L
template <class Rule, bool LATE>
struct ApplySink {
    cffm_tables_t w, s;
    int K, D;
    Rule rule;
    float gscale = 1.f;           // LATE only
    struct At { float *w, *s; };
    struct Pre { float w, s; };
    __device__ __forceinline__ At at(int id, int t, int col) const {
        const int64_t o = row_off(K, D, id, t, col);
        return {table_of(w, t) + o, rule.slot() ? table_of(s, t) + o : nullptr};
    }
    __device__ __forceinline__ Pre pre(const At& a) const { return {*a.w, rule.slot() ? *a.s : 0.f}; }
    __device__ __forceinline__ void operator()(const At& a, const Pre& p, float g) const {
        if (LATE) g *= gscale;
        float wv = p.w, sv = p.s;
        rule(wv, &sv, nullptr, g);                  // (a rule without a slot does not touch sv)
        if (rule.slot()) *a.s = sv;
        *a.w = wv;
    }
};
// store into the dense [M][K] | [M][D] | [M] gradient image
struct StoreSink {
    cffm_tables_t G;
    int K, D;
    typedef float* At;
    struct Pre {};
    __device__ __forceinline__ At at(int id, int t, int col) const { return table_of(G, t) + row_off(K, D, id, t, col); }
    __device__ __forceinline__ Pre pre(At) const { return {}; }
    __device__ __forceinline__ void operator()(At a, const Pre&, float g) const { *a = g; }
};
// the tables of store_mask (bit t = table t) have a dense gradient (Adam's non-lazy sparse apply; the regularised loss): their
// sums go to G* and dense_opt_kernel sweeps every row; the others are applied here, with no late scale
template <class Rule>
struct MixSink {
    ApplySink<Rule, false> apply;
    StoreSink store;
    int store_mask;
    struct At { typename ApplySink<Rule, false>::At a; float* G; };
    __device__ __forceinline__ At at(int id, int t, int col) const {
        if ((store_mask >> t) & 1) return {{nullptr, nullptr}, store.at(id, t, col)};
        return {apply.at(id, t, col), nullptr};
    }
    typedef typename ApplySink<Rule, false>::Pre Pre;
    __device__ __forceinline__ Pre pre(const At& a) const { return a.G ? Pre{0.f, 0.f} : apply.pre(a.a); }
    __device__ __forceinline__ void operator()(const At& a, const Pre& p, float g) const {
        if (a.G) store(a.G, StoreSink::Pre(), g);
        else apply(a.a, p, g);
    }
};

// the tables and slots of a sparse update with the late 1/L (the host half of ApplySink<Rule, true>)
struct ApplyArgs { cffm_tables_t w, s; LateScale ls; };
template <class Rule>
__device__ __forceinline__ void sparse_apply_body(int bid, const SparseArgs& a, const ApplyArgs& p, const Rule& rule) {
    segment_walk(bid, a, ApplySink<Rule, true>{p.w, p.s, a.K, a.D, rule, late_scale(p.ls)});
}
template <class Rule>
__global__ __launch_bounds__(256) void sparse_apply_kernel(SparseArgs a, ApplyArgs p, Rule rule) { sparse_apply_body(blockIdx.x, a, p, rule); }

// The two halves of the update do not depend on each other (dense slabs vs table rows): one launch, two roles.
__global__ __launch_bounds__(256) void update_all_kernel(const float* __restrict__ gpart, int64_t n, SlabPlan sp,
                                                         float* __restrict__ grad, float* __restrict__ theta,
                                                         float* __restrict__ acc, float lr, int n_reduce, SparseArgs sa, ApplyArgs pa) {
    if ((int)blockIdx.x < n_reduce) {
        PHASE_MARKB(26, blockIdx.x);
        reduce_slabs_body(blockIdx.x, gpart, n, sp, grad, theta, acc, lr);
        PHASE_MARKB(27, blockIdx.x);
    } else {
        PHASE_MARKB(28, blockIdx.x - n_reduce);
        sparse_apply_body(blockIdx.x - n_reduce, sa, pa, AdagradRule{lr});
        PHASE_MARKB(29, blockIdx.x - n_reduce);
    }
}
#ifdef CFFM_PHASE_TIMERS
extern "C" int cffm_debug_upd_times(unsigned long long* host32) {
    return (int)hipMemcpyFromSymbol(host32, HIP_SYMBOL(cffm_bwd_times), sizeof(cffm_bwd_times));
}
#endif

extern "C" int cffm_reduce_slabs(const cffm_shape_t* s, void* ws, int32_t B, float* grad, void* stream) {
    int rc = check_shape(s);
    if (rc) return rc;
    return cffm_reduce_slabs_impl(StepCtx(s, B, nullptr, ws), grad, nullptr, nullptr, 0.f, (hipStream_t)stream);
}

int cffm_reduce_slabs_impl(const StepCtx& c, float* grad, float* theta, float* acc, float lr, hipStream_t stream) {
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)reduce_slab_wgs(c.tl.n)), dim3(256), 0, stream,
                       c.at<const float>(c.wl.gpart), (int64_t)c.tl.n, c.sp, grad, theta, acc, lr);
    CFFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cffm_dense_adagrad(float* theta, float* acc, const float* grad, int64_t n, float lr, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(dense_late_kernel<AdagradRule>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       theta, acc, grad, n, AdagradRule{lr}, LateScale::none(), (float*)nullptr);
    CFFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int cffm_sparse_adagrad(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* acc,
                                   const int32_t* ids, int64_t n_rows, const float* dEi, const float* dEo,
                                   const float* dfb, void* ws, int32_t B_ws, void* stream) {
    int rc = check_shape(s);
    if (rc) return rc;
    const StepCtx c(s, B_ws, nullptr, ws);               // (the sort returns before it touches the workspace where B_ws < 1)
    if ((rc = cffm_sort_keys_impl(c, ids, n_rows, SortOpts(), (hipStream_t)stream))) return rc;
    return cffm_sparse_apply(c, tab, acc, n_rows, RowGrads{dEi, dEo, dfb, s->K, s->D, 1}, LateScale::none(), (hipStream_t)stream);
}

int cffm_sort_keys_impl(const StepCtx& c, const int32_t* ids, int64_t n_rows, const SortOpts& o, hipStream_t st) {
    const cffm_shape_t* s = c.s;
    if (n_rows <= 0) return 0;
    if (n_rows > (int64_t)c.B * s->F) return CFFM_ERR_BAD_SHAPE;
    unsigned long long* keys_in = c.at<unsigned long long>(c.wl.sort_keys);     // (id << 32) | slot
    unsigned long long* keys_out = c.at<unsigned long long>(c.wl.sort_vals);
    void* tmp = c.at<void>(c.wl.sort_tmp);
    size_t tmp_bytes = 0;
    const int bits = id_key_bits(s->M);
    // slots are unique, so sorting the packed keys IS the stable sort by id with slots ascending inside a segment
    if (!o.prepacked) {
        hipLaunchKernelGGL(pack_keys_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, ids, keys_in, n_rows, o.id_stride, s->M);
        CFFM_CHECK_LAUNCH();
    }
    if (n_rows <= 4096) {                       // one workgroup, one launch
        {
            hipError_t e0 = hipFuncSetAttribute((const void*)small_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SMALL_SORT_LDS);
            if (e0 != hipSuccess) return (int)e0;
        }
        hipLaunchKernelGGL(small_sort_kernel, dim3(1), dim3(256), SMALL_SORT_LDS, st, keys_in, keys_out, (int)n_rows, bits);
        CFFM_CHECK_LAUNCH();
        return 0;
    }
    hipError_t e = rocprim::radix_sort_keys((void*)nullptr, tmp_bytes, keys_in, keys_out, (size_t)n_rows, 0u,
                                            (unsigned)(32 + bits), st);
    if (e != hipSuccess) return (int)e;
    if (tmp_bytes > (size_t)c.wl.sort_tmp_bytes) return CFFM_ERR_BAD_SHAPE;
    e = rocprim::radix_sort_keys(tmp, tmp_bytes, keys_in, keys_out, (size_t)n_rows, 0u, (unsigned)(32 + bits), st);
    return e == hipSuccess ? 0 : (int)e;
}

SparseArgs StepCtx::sparse_args(int64_t n_rows, const RowGrads& r) const {
    SparseArgs a{};                       // run_len = 0: the slots address one array (dp_apply sets the run members for its blocks)
    a.keys = at<const unsigned long long>(wl.sort_vals);
    a.n = n_rows; a.M = s->M; a.K = s->K; a.D = s->D;
    a.dEi = r.dEi; a.dEo = r.dEo; a.dfb = r.dfb;
    a.sEi = r.sEi; a.sEo = r.sEo; a.sfb = r.sfb;
    return a;
}

int cffm_sparse_apply(const StepCtx& c, const cffm_tables_t* tab, const cffm_tables_t* acc, int64_t n_rows, const RowGrads& r,
                      const LateScale& ls, hipStream_t st) {
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(sparse_apply_kernel<AdagradRule>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, c.sparse_args(n_rows, r),
                       ApplyArgs{*tab, *acc, ls}, AdagradRule{c.s->lr});
    CFFM_CHECK_LAUNCH();
    return 0;
}

// fused single-GPU update: slab reduction + dense Adagrad and the sparse table update in one launch
int cffm_update_all(const StepCtx& c, const cffm_tables_t* tab, const cffm_tables_t* tab_acc, float* theta, float* theta_acc,
                    float* grad, hipStream_t st) {
    const int64_t n_rows = (int64_t)c.B * c.s->F;
    const int n_reduce = reduce_slab_wgs(c.tl.n);
    hipLaunchKernelGGL(update_all_kernel, dim3((unsigned)(n_reduce + (n_rows + 3) / 4)), dim3(256), 0, st,
                       c.at<const float>(c.wl.gpart), (int64_t)c.tl.n, c.sp, grad, theta, theta_acc, c.s->lr, n_reduce,
                       c.sparse_args(n_rows, RowGrads::of_ws(c)), ApplyArgs{*tab, *tab_acc, LateScale::none()});
    CFFM_CHECK_LAUNCH();
    return 0;
}

// Data-parallel apply (cffm_amd/dist.py): grad_sum = all-reduced [theta.n gradients | pad | loss-term sum at index
// theta.n], rows = all-gathered packed rows [n_rows][1 + K + D + 1] = (id bits | dEi | dEo | dfb).
// What both entry points do after their own refusals, for a rule that is, like Adagrad, a dense rule on theta and a
// duplicates-summed-first rule on the looked-up rows only (TF does not decay the Momentum accumulator of a row nobody looked up):
// dense rule with the late 1/L ∥ key placement or run merge (or the radix sort), then the segment walk with the applying sink.
// Every check comes before the first launch: a refused call has launched nothing.  slot / th1: the rule's first slot (NULL: none kept).
template <class Rule>
static int dp_apply(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* slot, float* theta, float* th1,
                    const float* grad_sum, int64_t B_global, const float* rows, int64_t n_rows, void* ws, int32_t B_ws, float* loss_out,
                    int32_t n_runs, const Rule& rule, bool needs_slot, hipStream_t st) {
    int rc;
    if (n_runs > 0) {
        // sorted runs (one per rank, from cffm_dp_local): merge by rank, rows addressed block-wise
        if (n_rows <= 0 || n_rows % n_runs || n_rows > (int64_t)B_ws * s->F || n_rows * 4 > CFFM_LDS_SHARED_CU) return CFFM_ERR_BAD_SHAPE;
        const int64_t m = n_rows / n_runs;
        if (m % s->F || !cffm_fwd_all_ok(s, (int32_t)(m / s->F))) return CFFM_ERR_UNSUPPORTED;      // the runs only exist on that path
    } else if (n_rows > 0 && n_rows > (int64_t)B_ws * s->F) {
        return CFFM_ERR_BAD_SHAPE;
    }
    if (!tab || !theta || !grad_sum || (n_rows > 0 && (!rows || !ws)) || (needs_slot && (!slot || !th1))) return CFFM_ERR_BAD_SHAPE;
    // B_ws < 1: n_rows <= 0 here, and nothing below touches the workspace
    const StepCtx c(s, B_ws, theta, ws);
    const cffm_theta_layout_t& tl = c.tl;
    const LateScale ls = {grad_sum + tl.n, 1.f / (float)B_global, s->loss == CFFM_LOSS_SQUARE_RMSE ? 1 : 0};
    const int64_t W = 1 + s->K + s->D + 1;
    const int n_dense = (int)((tl.n + 255) / 256);
    SparseArgs a = c.sparse_args(n_rows, RowGrads::packed(s, rows, W));
    if (n_runs > 0) {
        const int m = (int)(n_rows / n_runs);
        MergeArgs ma;
        ma.rows = rows; ma.block_floats = (int64_t)m * (W + 2); ma.keys_off = (int64_t)m * W; ma.m = m; ma.n_runs = n_runs;
        ma.out = c.at<unsigned long long>(c.wl.sort_vals);
        const size_t lds = (size_t)n_rows * 4;
        if ((rc = set_lds(dp_head_merge_kernel<Rule>, lds))) return rc;
        hipLaunchKernelGGL(dp_head_merge_kernel<Rule>, dim3(n_dense + (unsigned)((n_rows + 255) / 256)), dim3(256), lds, st, theta, th1,
                           grad_sum, (int64_t)tl.n, rule, ls, loss_out, n_dense, ma);
        CFFM_CHECK_LAUNCH();
        a.run_len = m; a.run_stride = ma.block_floats; a.inv_run_len = 1.f / (float)m;
    } else if (n_rows > 0 && n_rows <= 8192) {
        // dense update and key placement are independent: one launch, two roles
        const int n_rank = 256;                              // kpw = ceil(n_rows / 256) <= 32 keys per workgroup
        hipLaunchKernelGGL(dp_head_kernel<Rule>, dim3(n_dense + n_rank), dim3(256), 0, st, theta, th1, grad_sum, (int64_t)tl.n, rule, ls,
                           loss_out, n_dense, (const int32_t*)rows, W, (int)n_rows, n_rank, c.at<unsigned long long>(c.wl.sort_vals));
        CFFM_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL(dense_late_kernel<Rule>, dim3((unsigned)n_dense), dim3(256), 0, st, theta, th1, grad_sum, (int64_t)tl.n, rule,
                           ls, loss_out);
        CFFM_CHECK_LAUNCH();
        if (n_rows <= 0) return 0;
        SortOpts so;
        so.id_stride = W;                                    // the id column of the rows
        if ((rc = cffm_sort_keys_impl(c, (const int32_t*)rows, n_rows, so, st))) return rc;
    }
    hipLaunchKernelGGL(sparse_apply_kernel<Rule>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, a,
                       ApplyArgs{*tab, needs_slot ? *slot : NO_TABLES, ls}, rule);
    CFFM_CHECK_LAUNCH();
    return 0;
}

// Data-parallel apply (cffm_amd/dist.py): grad_sum = all-reduced [theta.n gradients | pad | loss-term sum at index
// theta.n], rows = all-gathered packed rows [n_rows][1 + K + D + 1] = (id bits | dEi | dEo | dfb).
extern "C" int cffm_dp_apply(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* acc, float* theta,
                             float* theta_acc, const float* grad_sum, int64_t B_global, const float* rows,
                             int64_t n_rows, void* ws, int32_t B_ws, float* loss_out, int32_t n_runs, void* stream) {
    int rc = check_shape(s);
    if (rc) return rc;
    if (s->optimizer != CFFM_OPT_ADAGRAD) return CFFM_ERR_UNSUPPORTED;    // the other rules: cffm_dp_apply_opt
    return dp_apply(s, tab, acc, theta, theta_acc, grad_sum, B_global, rows, n_rows, ws, B_ws, loss_out, n_runs, AdagradRule{s->lr}, true,
                    (hipStream_t)stream);
}

// SGD and Momentum for the data-parallel and row-sharded steps (acc / theta_acc = the Momentum accumulators; SGD reads neither).
// Adam is not here: TF's sparse Adam is non-lazy (every row of every table moves every step).
extern "C" int cffm_dp_apply_opt(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* acc, float* theta,
                                 float* theta_acc, const float* grad_sum, int64_t B_global, const float* rows,
                                 int64_t n_rows, void* ws, int32_t B_ws, float* loss_out, int32_t n_runs, void* stream) {
    int rc = check_shape(s);
    if (rc) return rc;
    if (s->optimizer == CFFM_OPT_ADAGRAD)
        return cffm_dp_apply(s, tab, acc, theta, theta_acc, grad_sum, B_global, rows, n_rows, ws, B_ws, loss_out, n_runs, stream);
    if (s->optimizer == CFFM_OPT_ADAM) return CFFM_ERR_UNSUPPORTED;       // non-lazy: a dense sweep of every table, not this design
    const bool mom = s->optimizer == CFFM_OPT_MOMENTUM;
    return dp_apply(s, tab, acc, theta, mom ? theta_acc : nullptr, grad_sum, B_global, rows, n_rows, ws, B_ws, loss_out, n_runs,
                    opt_rule(s, 1), mom, (hipStream_t)stream);
}

// ---- data-parallel step for SMALL vocabularies: the tables' gradients travel as one dense buffer --------------------
// When M*(K+D+1) floats are fewer than what all ranks' row gradients add up to (frappe: 350 K floats against
// N * 174 K), each rank scatters its duplicates-summed row gradients into a zeroed dense [M][K | D | 1] image that
// rides behind the dense-parameter gradient in ONE all-reduce; afterwards every rank sweeps the whole tables.  Rows
// nobody looked up carry an exact 0: acc + 0*0 and w - lr*0/sqrt(acc) leave them bit-identical, which is TF's sparse
// semantics without a mask.  flat = [theta.n gradients | loss sum | pad to n4 | Gi M*K | Go M*D | Gfb M].
static inline int64_t dp_dense_table_off(const cffm_theta_layout_t& tl) { return ((int64_t)tl.n + 4 + 3) / 4 * 4; }

struct LossSumArgs { const float* sqerr; int B; float *sum_dst, *scalars; };
__global__ __launch_bounds__(256) void dp_tail_dense_kernel(const float* __restrict__ gpart, int64_t n, SlabPlan sp,
                                                            float* __restrict__ grad, int n_reduce, SparseArgs sa, StoreSink sink,
                                                            LossSumArgs l) {
    __shared__ float red[4];
    const int bid = blockIdx.x - n_reduce;
    if (bid < 0) {
        reduce_slabs_body(blockIdx.x, gpart, n, sp, grad, nullptr, nullptr, 0.f);
    } else if (bid == 0) {                           // loss-term sum of this rank, fixed order
        float part = 0.f;
        for (int i = threadIdx.x; i < l.B; i += 256) part += l.sqerr[i];
        const float sum = block_sum(part, red);
        if (threadIdx.x == 0) { l.sum_dst[0] = sum; l.scalars[0] = sum; }
    } else {
        segment_walk(bid - 1, sa, sink);
    }
}

int cffm_dp_tail_dense(const StepCtx& c, float* flat, hipStream_t st) {
    const cffm_shape_t* s = c.s;
    const cffm_theta_layout_t& tl = c.tl;
    const cffm_ws_layout_t& wl = c.wl;
    const int64_t n_rows = (int64_t)c.B * s->F;
    float* Gi = flat + dp_dense_table_off(tl);
    float* Go = Gi + (int64_t)s->M * s->K;
    const StoreSink sink = {{Gi, Go, Go + (int64_t)s->M * s->D}, s->K, s->D};
    const LossSumArgs l = {c.at<const float>(wl.sqerr), c.B, flat + tl.n, c.at(wl.scalars)};
    const int n_reduce = reduce_slab_wgs(tl.n);
    const int n_scatter = 1 + (int)((n_rows + 3) / 4);
    hipLaunchKernelGGL(dp_tail_dense_kernel, dim3(n_reduce + n_scatter), dim3(256), 0, st, c.at<const float>(wl.gpart),
                       (int64_t)tl.n, c.sp, flat, n_reduce, c.sparse_args(n_rows, RowGrads::of_ws(c)), sink, l);   // both branches are on (cffm_fwd_all_ok)
    CFFM_CHECK_LAUNCH();
    return 0;
}

struct DenseTableArgs { float *w[3], *a[3]; float* g[3]; int64_t n[3]; };
__global__ __launch_bounds__(256) void dp_apply_dense_kernel(float* __restrict__ v, float* __restrict__ acc, const float* __restrict__ grad,
                                                             int64_t n, float lr, LateScale ls, float* __restrict__ loss_out, int n_dense,
                                                             DenseTableArgs t) {
    const AdagradRule rule = {lr};
    if ((int)blockIdx.x < n_dense) { dense_late_body(blockIdx.x, v, acc, grad, n, rule, ls, loss_out); return; }
    int64_t i = (int64_t)(blockIdx.x - n_dense) * 256 + threadIdx.x;
    const float gs = late_scale(ls);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (i < t.n[k]) {
            const float g = t.g[k][i] * gs;
            t.g[k][i] = 0.f;                                 // zero on exit: the next step's scatter finds a clean image (no memset)
            rule(t.w[k][i], t.a[k] + i, nullptr, g);         // g == 0 (row not looked up by any rank): a and w unchanged
            return;
        }
        i -= t.n[k];
    }
}

extern "C" int64_t cffm_dp_dense_floats(const cffm_shape_t* s) {
    if (check_shape(s)) return -1;
    cffm_theta_layout_t tl;
    cffm_theta_layout(s, &tl);
    return dp_dense_table_off(tl) + (int64_t)s->M * (s->K + s->D + 1);
}

extern "C" int cffm_dp_apply_dense(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* acc, float* theta,
                                   float* theta_acc, float* flat_sum, int64_t B_global, float* loss_out, void* stream) {
    int rc = check_shape(s);
    if (rc) return rc;
    if (s->optimizer != CFFM_OPT_ADAGRAD) return CFFM_ERR_UNSUPPORTED;    // as cffm_dp_apply
    if (!s->inner_conv || !s->outer_conv) return CFFM_ERR_UNSUPPORTED;
    cffm_theta_layout_t tl;
    cffm_theta_layout(s, &tl);
    const int64_t toff = dp_dense_table_off(tl);
    LateScale ls = {flat_sum + tl.n, 1.f / (float)B_global, s->loss == CFFM_LOSS_SQUARE_RMSE ? 1 : 0};
    DenseTableArgs t;
    t.w[0] = tab->inner_emb; t.w[1] = tab->outer_emb; t.w[2] = tab->feat_bias;
    t.a[0] = acc->inner_emb; t.a[1] = acc->outer_emb; t.a[2] = acc->feat_bias;
    t.n[0] = (int64_t)s->M * s->K; t.n[1] = (int64_t)s->M * s->D; t.n[2] = s->M;
    t.g[0] = flat_sum + toff; t.g[1] = t.g[0] + t.n[0]; t.g[2] = t.g[1] + t.n[1];
    const int n_dense = (int)((tl.n + 255) / 256);
    const int64_t nt = t.n[0] + t.n[1] + t.n[2];
    hipLaunchKernelGGL(dp_apply_dense_kernel, dim3((unsigned)(n_dense + (nt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, theta,
                       theta_acc, flat_sum, (int64_t)tl.n, s->lr, ls, loss_out, n_dense, t);
    CFFM_CHECK_LAUNCH();
    return 0;
}

// ---- tables with a dense gradient: Adam's non-lazy sparse apply and the regularised square loss (CFFM.py:489-491) ----------------
// lam != 0: the l2_regularizer term of the regularised square loss, g = grad + lam * w
template <class Rule>
__global__ __launch_bounds__(256) void dense_opt_kernel(float* __restrict__ w, float* __restrict__ s1, float* __restrict__ s2,
                                                        const float* __restrict__ grad, int64_t n, Rule rule, float lam) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float wv = w[i];
    rule(wv, s1 ? s1 + i : nullptr, s2 ? s2 + i : nullptr, (grad ? grad[i] : 0.f) + lam * wv);
    w[i] = wv;
}

// the rule on the touched rows (duplicates summed first, in slot order), except the tables of MixSink::store_mask
template <class Rule>
__global__ __launch_bounds__(256) void sparse_mix_kernel(SparseArgs a, MixSink<Rule> sink) { segment_walk(blockIdx.x, a, sink); }

// The table update of the single-GPU step from the packed keys in ws.sort_keys.  Adam: TF's sparse Adam is non-lazy, so the summed
// rows of all three tables go to zeroed dense buffers G* and a dense sweep moves every row.  Regularised square loss: the l2 terms
// make the gradients of the two embedding tables dense for every optimizer (IndexedSlices + dense aggregates to dense), g = G +
// lamda * w; feature_bias stays sparse.  Otherwise: the rule on the touched rows only.
template <class Rule>
static int tables_apply(const StepCtx& cx, const cffm_tables_t* tab, const cffm_tables_t& t1, const cffm_tables_t& t2, int64_t n_rows,
                        const Rule& rule, bool adam, hipStream_t st) {
    const cffm_shape_t* s = cx.s;
    const cffm_ws_layout_t& wl = cx.wl;
    const bool l2 = s->loss == CFFM_LOSS_SQUARE_L2;
    const int store_mask = adam ? 7 : (l2 ? 3 : 0);
    const cffm_tables_t G = store_mask ? cffm_tables_t{cx.at(wl.Gi), cx.at(wl.Go), cx.at(wl.Gfb)} : NO_TABLES;
    const int64_t ni = (int64_t)s->M * s->K, no = (int64_t)s->M * s->D, nf = s->M;
    if (store_mask) {
        hipError_t e = hipMemsetAsync(G.inner_emb, 0, (size_t)(wl.Gfb + nf * 4 - wl.Gi), st);     // the three buffers are contiguous
        if (e != hipSuccess) return (int)e;
    }
    SortOpts so;
    so.prepacked = true;
    int rc = cffm_sort_keys_impl(cx, nullptr, n_rows, so, st);
    if (rc) return rc;
    hipLaunchKernelGGL(sparse_mix_kernel<Rule>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, cx.sparse_args(n_rows, RowGrads::of_ws(cx)),
                       MixSink<Rule>{{*tab, t1, s->K, s->D, rule}, {G, s->K, s->D}, store_mask});
    CFFM_CHECK_LAUNCH();
    if (store_mask) {      // dense sweeps; a disabled branch has no table variable and is left alone
        if (s->inner_conv)
            hipLaunchKernelGGL(dense_opt_kernel<Rule>, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, st, tab->inner_emb, t1.inner_emb,
                               t2.inner_emb, (const float*)G.inner_emb, ni, rule, l2 ? s->lamda : 0.f);
        if (s->outer_conv)
            hipLaunchKernelGGL(dense_opt_kernel<Rule>, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, st, tab->outer_emb, t1.outer_emb,
                               t2.outer_emb, (const float*)G.outer_emb, no, rule, l2 ? s->lamda_att : 0.f);    // quirk Q13: lamda_att scales the outer table
        if (adam)
            hipLaunchKernelGGL(dense_opt_kernel<Rule>, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, tab->feat_bias, t1.feat_bias,
                               t2.feat_bias, (const float*)G.feat_bias, nf, rule, 0.f);
        CFFM_CHECK_LAUNCH();
    }
    return 0;
}

// Adagrad under the regularised square loss (theta was updated with the slab reduction)
int cffm_tables_adagrad_l2(const StepCtx& c, const cffm_tables_t* tab, const cffm_tables_t* acc, int64_t n_rows, hipStream_t st) {
    return tables_apply(c, tab, *acc, NO_TABLES, n_rows, AdagradRule{c.s->lr}, false, st);
}

int cffm_apply_opt(const StepCtx& cx, const cffm_tables_t* tab, const cffm_tables_t* st1, const cffm_tables_t* st2, float* theta,
                   float* th1, float* th2, const float* grad, int64_t n_rows, int64_t step, hipStream_t st) {
    const OptRule rule = opt_rule(cx.s, step);
    hipLaunchKernelGGL(dense_opt_kernel<OptRule>, dim3((unsigned)((cx.tl.n + 255) / 256)), dim3(256), 0, st, theta, th1, th2, grad,
                       (int64_t)cx.tl.n, rule, 0.f);
    CFFM_CHECK_LAUNCH();
    return tables_apply(cx, tab, st1 ? *st1 : NO_TABLES, st2 ? *st2 : NO_TABLES, n_rows, rule, rule.c.opt == CFFM_OPT_ADAM, st);
}

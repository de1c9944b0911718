// Embedding tables drawn BY GLOBAL ROW (cffm_init_table_rows, include/cffm_hip.h): a value is a function of
// (seed, global row, table, column) alone, so a row-sharded rank that owns rows r, r + G, ... draws exactly the rows a
// single process would hold there, whatever the world size.  The reference draws its tables with tf.random_normal
// (CFFM.py:257-277: N(0, 0.1), N(0, 0.01), exact zeros) from an unseeded graph; the distributions are kept, the stream is ours.
//
//   counter-based generator: Philox4x32-10, key = (seed lo, seed hi), counter = (row lo, row hi, q, t) with q the group of four
//   columns and t the table (0 inner, 1 outer); the four output words become four normals by two Box-Muller pairs on 24-bit
//   uniforms (exact in fp32).  cffm_amd/spec.py table_rows() is the numpy twin and the specification.
//
// Pure write stream: one thread per four-column group, consecutive threads on consecutive groups of one row (the inner groups
// of the row, then its outer groups), one 16-byte store per thread where the row pitch keeps the groups 16-byte aligned
// (width % 4 == 0), two 8-byte stores otherwise (the widths are even).  Grid-stride over the groups with the (row, group) pair
// advanced incrementally, so the loop holds no 64-bit division; no LDS, 36 VGPRs (8 waves per SIMD), nothing but occupancy to hide the stores.
#include "internal.hpp"
#include "philox.hpp"

#define INIT_THREADS 256
#define INIT_MAX_BLOCKS 2048            // 256 CUs x 8 blocks: a memory-bound grid is capped there and strides the rest

struct InitArgs {
    float* tab[2];                      // inner, outer (nullptr: branch disabled, no groups)
    int width[2];                       // K, D
    uint32_t groups[2];                 // four-column groups per row of each table (0 for a disabled branch)
    int vec16[2];                       // 16-byte stores allowed
    uint32_t k0, k1;
    uint64_t row0, row_step, n_rows;
    uint64_t step_rows;                 // the grid stride (gridDim.x * INIT_THREADS groups) as rows + leftover groups
    uint32_t step_groups;
};

// two unit normals from two words: u1 in (0, 1], u2 in [0, 1), both multiples of 2^-24
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(b >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);     // the angle 2 pi u2 without rounding 2 pi u2 itself
    z0 = r * cs; z1 = r * sn;
}

__global__ __launch_bounds__(INIT_THREADS) void init_table_rows_kernel(InitArgs a) {
    const uint32_t gt = a.groups[0] + a.groups[1];
    const uint64_t w0 = (uint64_t)blockIdx.x * INIT_THREADS + threadIdx.x;
    uint64_t l = w0 / gt;                                   // local row (the only division of the thread)
    uint32_t j = (uint32_t)(w0 - l * gt);                   // group inside the row: inner groups first
    while (l < a.n_rows) {
        const int t = j >= a.groups[0] ? 1 : 0;
        const uint32_t q = t ? j - a.groups[0] : j;
        const uint64_t g = a.row0 + l * a.row_step;         // global row
        uint32_t x[4];
        philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), q, (uint32_t)t, a.k0, a.k1, x);
        float z0, z1, z2, z3;
        box_muller(x[0], x[1], z0, z1);
        box_muller(x[2], x[3], z2, z3);
        const float sc = t ? 0.01f : 0.1f;
        const int width = a.width[t];
        float* p = a.tab[t] + l * (uint64_t)width + 4u * q;
        if (a.vec16[t]) {
            *reinterpret_cast<float4*>(p) = make_float4(sc * z0, sc * z1, sc * z2, sc * z3);
        } else {
            *reinterpret_cast<float2*>(p) = make_float2(sc * z0, sc * z1);
            if ((int)(4u * q) + 4 <= width)                 // the last group of a width % 4 == 2 row keeps two columns
                *reinterpret_cast<float2*>(p + 2) = make_float2(sc * z2, sc * z3);
        }
        l += a.step_rows;
        j += a.step_groups;
        if (j >= gt) { j -= gt; ++l; }
    }
}

extern "C" int cffm_init_table_rows(const cffm_shape_t* s, const cffm_tables_t* tab, uint64_t seed, int64_t row0, int64_t row_step,
                                    int64_t n_rows, void* stream) {
    // not check_shape(): that wants K % 4 == 0 for the float4 rows of the step kernels; the draw only needs even widths
    if (!s || !tab || s->M < 1 || s->K < 2 || (s->K & 1) || s->D < 2 || (s->D & 1)) return CFFM_ERR_BAD_SHAPE;
    if (row0 < 0 || row_step < 1 || n_rows < 0 || n_rows > (int64_t)s->M) return CFFM_ERR_BAD_SHAPE;
    if ((s->inner_conv && !tab->inner_emb) || (s->outer_conv && !tab->outer_emb)) return CFFM_ERR_BAD_SHAPE;
    if (n_rows > 1 && (n_rows - 1) > (INT64_MAX - row0) / row_step) return CFFM_ERR_BAD_SHAPE;     // the last global row overflows
    InitArgs a;
    a.tab[0] = s->inner_conv ? tab->inner_emb : nullptr;
    a.tab[1] = s->outer_conv ? tab->outer_emb : nullptr;
    a.width[0] = s->K; a.width[1] = s->D;
    for (int t = 0; t < 2; ++t) {
        const uintptr_t addr = reinterpret_cast<uintptr_t>(a.tab[t]);
        if (addr & 7) return CFFM_ERR_BAD_SHAPE;            // 8-byte stores at the least
        a.groups[t] = a.tab[t] ? (uint32_t)((a.width[t] + 3) / 4) : 0u;
        a.vec16[t] = (a.width[t] % 4 == 0 && (addr & 15) == 0) ? 1 : 0;
    }
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (tab->feat_bias) {                                   // random_normal(stddev = 0), CFFM.py:276: exact zeros
        hipError_t e = hipMemsetAsync(tab->feat_bias, 0, (size_t)n_rows * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
    }
    const uint32_t gt = a.groups[0] + a.groups[1];
    if (gt == 0) return 0;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.row0 = (uint64_t)row0; a.row_step = (uint64_t)row_step; a.n_rows = (uint64_t)n_rows;
    const uint64_t total = (uint64_t)n_rows * gt;
    const uint64_t want = (total + INIT_THREADS - 1) / INIT_THREADS;
    const uint32_t blocks = (uint32_t)(want < INIT_MAX_BLOCKS ? want : INIT_MAX_BLOCKS);
    const uint64_t stride = (uint64_t)blocks * INIT_THREADS;
    a.step_rows = stride / gt;
    a.step_groups = (uint32_t)(stride % gt);
    hipLaunchKernelGGL(init_table_rows_kernel, dim3(blocks), dim3(INIT_THREADS), 0, st, a);
    CFFM_CHECK_LAUNCH();
    return 0;
}

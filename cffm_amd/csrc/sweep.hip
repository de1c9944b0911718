// Candidate sweep with the fixed-field work done once per context.
//
// cffm_score_sweep scores C contexts x N candidates: row c is context ctx[c] with its id at `field` replaced by every candidate in
// turn.  cffm_predict on the expanded id rows (engine.score_candidates) treats the C * N rows as unrelated; here everything that
// does not change with the candidate is computed once per context and only the rest runs per candidate.
//
// Notation of conv0_fact_fwd_body (conv.hip): f = the swept field, E_i = the outer row of context field i, e = the candidate's
// outer row, W[dh][dw][(i,j)][q] the layer-0 filter, b its bias, (y, x) the output pixel, q the output channel.  The layer-0
// pre-activation splits exactly into
//     Z[y][x][q] = b[q] + Zctx[y][x][q] + sum_dw e[2x+dw] * U[dw][y][q] + sum_dh e[2y+dh] * V[dh][x][q]
//     Zctx[y][x][q] = sum over pairs (i,j), i != f, j != f, of sum_dh sum_dw E_i[2y+dh] * E_j[2x+dw] * W[dh][dw][(i,j)][q]
//     U[dw][y][q]   = sum_dh sum_{i<f} E_i[2y+dh] * W[dh][dw][(i,f)][q]       pairs (i,f): the candidate is the column operand
//     V[dh][x][q]   = sum_dw sum_{j>f} E_j[2x+dw] * W[dh][dw][(f,j)][q]       pairs (f,j): the T plane (dh, f) of conv0_fact_fwd
// (U carries its sum over dh already: e[2x+dw] does not depend on dh).  Zctx, U and V depend on the context alone: per candidate
// layer 0 is 4 multiply-adds per output element and needs no filter.  The inner branch is a plain sum over pairs, so the terms
// of the pairs without f are one number per context; the s0 pool splits into s0fix[h] + A[h] * rowsum(e) + e[h] * R with
// A[h] = sum_{i<f} E_i[h], R = sum_{j>f} rowsum(E_j).  Everything above layer 0 is per candidate (act(relu(Z)) is not linear).
//
// Two launches on the caller's stream:
//   sweep_ctx_kernel   one workgroup (256 threads) per context: gathers the context's rows (ids clamped as the forward clamps them),
//                      runs the factorised layer 0 of conv0_fact_fwd_body on v_mfma_f32_16x16x4_f32 with embedding row f zeroed and
//                      the epilogue taken before bias and relu (Zctx), keeps its T planes (dh, f) (V), contracts the mirrored step 1
//                      over i < f (U), and leaves them with the fixed inner sum, the s0 parts, the inner rows and the fb row in the
//                      context's block of the caller's scratch.
//   sweep_cand_kernel  workgroups of 512 threads take (context, chunk of CFFM_SWEEP_CHUNK candidates) units from a flat 1-D range:
//                      the parallelism is C * ceil(N / chunk).  Per unit the block is staged once: Zctx + b in registers (24 floats
//                      per thread at Pp = 48), U and V in LDS.  Per candidate: one inner row, one outer row and one feature_bias
//                      value (the next candidate's are requested before the current one's arithmetic), C_0 = relu(Z) in LDS, conv
//                      layers 1..3 on LDS-resident activations (layer 1's filter stays in LDS for the whole launch, every lane's B
//                      fragments of layers 2 and 3 in registers: no filter is read per candidate), the pools, dense 32 / 1, the first-order term, add_n, one float stored.
// The kernel boundary between the two orders the block writes before their reads.  Every barrier of both kernels sits in
// straight-line code or in a loop whose trip count is workgroup-uniform (a kernel argument or derived from blockIdx); the
// wave-uniform role branches between two barriers contain none.  Every reduction runs in a fixed order that depends on the
// thread mapping alone: a candidate's score is the same bits at every position of every chunk, on every call.
//
// Tuples (cffm_score_sweep_tuples): a candidate replaces nf <= CFFM_SWEEP_MAX_NF fields f_0 < f_1 < ... together
// (the host sorts the caller's list and hands the kernels the column permutation).  e_a = the candidate's outer row at f_a.  Every
// layer-0 pair (i, j), i < j, is of one of three classes:
//     neither swept     Zctx as above, with ALL swept rows of the embedding tile zero
//     one swept, f_a    U_a / V_a as above over the fields that are not swept: with the swept rows zero the step-1 contraction yields
//                       both, its T plane (dh, f_a) being V_a and its mirrored step 1 U_a
//     both, f_a < f_b   X_ab[y][x][q] = sum_dh sum_dw e_a[2y+dh] * e_b[2x+dw] * W[dh][dw][(f_a,f_b)][q]: per candidate, rank one; its
//                       4 Pp filter floats depend on theta alone and are staged once per workgroup
//     Z = b + Zctx + sum_a (sum_dw e_a[2x+dw] U_a[dw][y] + sum_dh e_a[2y+dh] V_a[dh][x]) + sum_{a<b} X_ab
//     s0[h] = s0fix[h] + sum_a (A_a[h] rowsum(e_a) + e_a[h] R_a) + sum_{a<b} e_a[h] rowsum(e_b),   A_a / R_a over the fields not swept
// The fixed inner sum keeps the pairs with no swept field; the per-candidate part runs over the list of all pairs with at least one;
// the first-order term takes the candidates' feature_bias at every swept slot.  The context role is one kernel for every nf (U_a
// on 2 nf wave roles over its four wavefronts; the block grows by U_a, V_a and A_a per field).  The candidate role is one code for
// every nf as well, with the field count a template parameter: NF = 1 for one field (cffm_score_sweep, _lists, and tuples of one: the
// loops over the swept fields unroll, the loop over the swept-swept pairs is empty) and NF = 0 for a.nf = 2 .. 4 at run time - two
// instances per Pp.  It stages all U_a / V_a and the swept-swept filter slices in LDS, builds the list of live pairs by a ballot (one
// straight-line barrier between the ballot and the gather of their dense(1) weights, for every instance), fetches nf inner rows,
// outer rows and biases ahead (one 16-byte piece per thread, nf (K/4 + D/4 + 1) threads; a candidate's bias goes to its field's slot
// of the feature_bias row), forms C_0 with 4 nf multiply-adds plus 4 per swept-swept pair and element - per field in sorted order,
// then the pairs (a < b) - adds s0 one term at a time per field (A_a rowsum(e_a), e_a R_a, then the fields below a), and from C_0 on
// runs the code above.  Its sums depend on the thread mapping and the sorted field order alone.  The one LDS formula (sweep_lds)
// decides what is served: one field up to K = 408 at F = 10, nf = 2 at every F <= 10 (at F = 10 up to K = 160), nf <= 4 at Pp <= 32;
// nf = 3 at Pp = 48 does not fit a CU.
#include <cstddef>
#include <cstring>

#include "inner_body.hpp"
#include "internal.hpp"

#define SWEEP_NTH 512                  // threads of a candidate workgroup
#define SWEEP_D 32                     // served outer dimension: C_0 16x16, C_1 8x8, C_2 4x4, C_3 2x2 (live = 4)
#define SWEEP_S 16
#define SWEEP_MAXPP 48                 // F <= 10
#define SWEEP_HEADER 256               // bytes of the scratch in front of the first context's block

namespace {

// per-context block of the scratch, offsets in floats (every one a multiple of 4)
struct SweepBlock {
    int Z, U, V, Ei, s0fix, A, fb, scal;    // scal: [0] fixed inner sum, [1 + a] R_a = sum_{j>f_a, j not swept} rowsum(E_j)
    int64_t floats;
};
__host__ __device__ inline SweepBlock sweep_block(int Pp, int F, int K, int nf = 1) {
    SweepBlock b;
    int o = 0;
    b.Z = o; o += SWEEP_S * SWEEP_S * Pp;   // [y][x][q]
    b.U = o; o += nf * 2 * SWEEP_S * Pp;    // [a][dw][y][q]
    b.V = o; o += nf * 2 * SWEEP_S * Pp;    // [a][dh][x][q]
    b.Ei = o; o += F * K;                   // inner rows, the swept rows zero
    b.s0fix = o; o += SWEEP_D;
    b.A = o; o += nf * SWEEP_D;             // [a][h]
    b.fb = o; o += 16;                      // feature_bias of the context's fields, the swept slots zero
    b.scal = o; o += 16;
    b.floats = (o + 63) / 64 * 64;
    return b;
}

__device__ __forceinline__ int sweep_clamp(int id, int M) { return id < 0 ? 0 : (id >= M ? M - 1 : id); }
__device__ __forceinline__ int sweep_pair(int i, int j, int F) { return i * (2 * F - i - 1) / 2 + j - i - 1; }   // i < j
// The swept fields travel by value, sorted, four bits each (F <= 10): a lane reads its own without indexing a kernel argument.
__device__ __forceinline__ int sweep_field(uint32_t packed, int a) { return (int)((packed >> (4 * a)) & 15u); }

// ---------------------------------------------------------------------------------------------------------------------------
// context role
// ---------------------------------------------------------------------------------------------------------------------------
struct SweepCtxArgs {
    Geo g;
    const float *inner, *outer, *fbias;
    const int32_t* ctx;
    int nf;                                // swept fields f_0 < f_1 < ... (one for cffm_score_sweep / _lists)
    uint32_t fields, swept;                // sweep_field(fields, a) = f_a; bit f of swept: field f is swept
    const float *W0, *cw, *cb, *wd;
    float* blocks;
    int64_t block_floats;
};

static inline size_t sweep_ctx_lds(int Pp, int F, int K) {
    const size_t TP = SWEEP_S * Pp + 16, EsN = ((size_t)F * (SWEEP_D + 1) + 3) / 4 * 4;
    return ((size_t)4 * Pp * Pp + 2 * F * TP + EsN + (size_t)F * K + Pp + 16 + 16) * 4;
}

template <int NT>
__global__ __launch_bounds__(256) void sweep_ctx_kernel(SweepCtxArgs a) {
    constexpr int PP = NT * 16, NW = 4, NTH = 64 * NW, D = SWEEP_D, S = SWEEP_S, Dp = D + 1, TP = S * PP + 16, XQ = 16 / NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Geo& g = a.g;
    const int F = g.F, K = g.K, nf = a.nf;
    const uint32_t sw = a.swept;
    const int EsN = (F * Dp + 3) / 4 * 4;
    float* Wl = reinterpret_cast<float*>(smem);                  // [4*PP][PP]
    float* T = Wl + 4 * PP * PP;                                 // [2F][TP]
    float* Es = T + 2 * F * TP;                                  // [F][Dp], the swept rows zero
    float* Ein = Es + EsN;                                       // [F][K], the swept rows zero
    uint32_t* lut = reinterpret_cast<uint32_t*>(Ein + F * K);    // [PP]
    float* rs = reinterpret_cast<float*>(lut + PP);              // [16]
    float* red = rs + 16;                                        // [16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kk = lane >> 4;
    const int32_t* idb = a.ctx + (int64_t)blockIdx.x * F;
    float* blk = a.blocks + (int64_t)blockIdx.x * a.block_floats;
    const SweepBlock bo = sweep_block(PP, F, K, nf);

    // ---- stage the filter, gather the context's rows (the swept rows of both tiles are zero: the candidate takes their place) ----
    for (int i = tid; i < PP * PP; i += NTH) reinterpret_cast<float4*>(Wl)[i] = reinterpret_cast<const float4*>(a.W0)[i];
    for (int i = tid; i < F * (D / 4); i += NTH) {
        const int fr = i / (D / 4), c4 = i - fr * (D / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!((sw >> fr) & 1u)) v = reinterpret_cast<const float4*>(a.outer)[(int64_t)sweep_clamp(idb[fr], g.M) * (D / 4) + c4];
        float* e = Es + fr * Dp + 4 * c4;
        e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
    }
    const int K4 = K / 4;
    for (int i = tid; i < F * K4; i += NTH) {
        const int fr = i / K4, c4 = i - fr * K4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!((sw >> fr) & 1u)) v = reinterpret_cast<const float4*>(a.inner)[(int64_t)sweep_clamp(idb[fr], g.M) * K4 + c4];
        reinterpret_cast<float4*>(Ein)[i] = v;
        reinterpret_cast<float4*>(blk + bo.Ei)[i] = v;
    }
    if (tid < 16) blk[bo.fb + tid] = (tid < F && !((sw >> tid) & 1u)) ? a.fbias[sweep_clamp(idb[tid], g.M)] : 0.f;
    build_pair_lut(lut, F, PP);
    const float cw[4] = {a.cw[0], a.cw[1], a.cw[2], a.cw[3]};
    const float cb[2] = {a.cb[0], a.cb[1]};
    __syncthreads();

    // ---- step 1 of the factorised layer 0 (conv0_fact_fwd_body, S = 16: one row tile): T[dh][i][x][q] ----
    const int units = 2 * (F - 1);
    for (int u = wave; u < units; u += NW) {
        const int i = u % (F - 1), dh = u / (F - 1);
        const int nj = F - 1 - i, Kc = 2 * nj;                  // k = dw * nj + (j - i - 1)
        const int base = i * (2 * F - i - 1) / 2;               // first pair (i, i+1)
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Kc; k0 += 4) {
            const int k = k0 + kk;
            const bool ok = k < Kc;
            const int dw = (ok && k >= nj) ? 1 : 0, jj = ok ? k - dw * nj : 0;
            const float av = ok ? Es[(i + 1 + jj) * Dp + 2 * r + dw] : 0.f;
            const float* wr = Wl + ((dh * 2 + dw) * PP + base + jj) * PP + r;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma16(av, ok ? wr[nt * 16] : 0.f, acc[nt]);
        }
        float* tp = T + (dh * F + i) * TP + r;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) tp[(kk * 4 + j) * PP + nt * 16] = acc[nt][j];
    }
    for (int e = tid; e < 2 * S * PP; e += NTH) {                // planes (dh, F-1) have no pairs
        const int dh = e / (S * PP), o = e - dh * (S * PP);
        T[(dh * F + F - 1) * TP + o] = 0.f;
    }
    // row sums of the outer rows (a swept row: 0)
    for (int i = wave; i < F; i += NW) {
        const float s = wave_sum(lane < D ? Es[i * Dp + lane] : 0.f);
        if (lane == 0) rs[i] = s;
    }
    lds_barrier();

    // ---- V_a = the T planes (dh, f_a): with the swept rows zero they hold the pairs (f_a, j), j not swept, alone ----
    for (int e = tid; e < nf * 2 * S * PP; e += NTH) {
        const int ad = e / (S * PP), o = e - ad * (S * PP), dh = ad & 1;
        blk[bo.V + e] = T[(dh * F + sweep_field(a.fields, ad >> 1)) * TP + o];
    }
    // ---- step 2 without bias and relu: Zctx (wave w owns x = 4w .. 4w+3) ----
    {
        const int K2 = 2 * F, ks2 = (K2 + 3) / 4, xg = wave * XQ;
        f32x4 acc[XQ][NT];
#pragma unroll
        for (int q4 = 0; q4 < XQ; ++q4)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[q4][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int s2 = 0; s2 < ks2; ++s2) {
            const int k = 4 * s2 + kk;
            const bool ok = k < K2;
            const int dh = (ok && k >= F) ? 1 : 0, i = ok ? k - dh * F : 0;
            const float av = ok ? Es[i * Dp + 2 * r + dh] : 0.f;
            const float* tb = T + (ok ? k : 0) * TP + xg * PP + r;
#pragma unroll
            for (int q4 = 0; q4 < XQ; ++q4)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[q4][nt] = mfma16(av, ok ? tb[q4 * PP + nt * 16] : 0.f, acc[q4][nt]);
        }
#pragma unroll
        for (int q4 = 0; q4 < XQ; ++q4)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j) blk[bo.Z + ((kk * 4 + j) * S + xg + q4) * PP + nt * 16 + r] = acc[q4][nt][j];
    }
    // ---- U_a[dw]: the mirrored step 1, rows y, k = (dh, i < f_a), the candidate being the column operand: 2 nf wave roles over the
    // four wavefronts (a swept i < f_a contributes exact zeros) ----
    for (int role = wave; role < 2 * nf; role += NW) {
        const int dw = role & 1, f = sweep_field(a.fields, role >> 1), Kf = 2 * f;
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Kf; k0 += 4) {
            const int k = k0 + kk;
            const bool ok = k < Kf;
            const int dh = (ok && k >= f) ? 1 : 0, i = ok ? k - dh * f : 0;
            const float av = ok ? Es[i * Dp + 2 * r + dh] : 0.f;
            const float* wr = Wl + ((dh * 2 + dw) * PP + (ok ? sweep_pair(i, f, F) : 0)) * PP + r;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma16(av, ok ? wr[nt * 16] : 0.f, acc[nt]);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) blk[bo.U + (role * S + kk * 4 + j) * PP + nt * 16 + r] = acc[nt][j];
    }
    // ---- the s0 pool: s0fix[h] = sum_{i<j, neither swept} E_i[h] * rowsum(E_j) (the swept rows of Es are zero), A_a[h], R_a ----
    if (tid < D) {
        float s = 0.f, R = 0.f;
        for (int i = F - 2; i >= 0; --i) {
            R += rs[i + 1];
            s += Es[i * Dp + tid] * R;
        }
        blk[bo.s0fix + tid] = s;
        for (int sa = 0; sa < nf; ++sa) {
            const int f = sweep_field(a.fields, sa);
            float A = 0.f;
            for (int i = 0; i < f; ++i) A += Es[i * Dp + tid];
            blk[bo.A + sa * D + tid] = A;
        }
    }
    if (tid < nf) {
        float R = 0.f;
        for (int j = sweep_field(a.fields, tid) + 1; j < F; ++j) R += rs[j];
        blk[bo.scal + 1 + tid] = R;
    }
    // ---- the inner-branch terms of the pairs without a swept field ----
    const int K2i = K / 2, nun = g.P * K2i;
    const float2* wd2 = reinterpret_cast<const float2*>(a.wd);
    float part = 0.f;
    for (int u = tid; u < nun; u += NTH) {
        const int p = u / K2i, t = u - p * K2i;
        const uint32_t ij = lut[p];
        if (((sw >> (ij & 0xffff)) | (sw >> (ij >> 16))) & 1u) continue;
        const InnerUnit v = inner_unit(Ein, lut, p, t, K, cw, cb, g.act);
        const float2 w2 = wd2[u];
        part += v.s0 * w2.x + v.s1 * w2.y;
    }
    const float tot = block_sum(part, red);
    if (tid == 0) blk[bo.scal] = tot;
}

// ---------------------------------------------------------------------------------------------------------------------------
// candidate role
// ---------------------------------------------------------------------------------------------------------------------------
struct SweepArgs {
    Geo g;
    int loss;
    const float *inner, *outer, *fbias;
    const int32_t* cand;
    int64_t cand_ctx_stride;               // elements between the lists of two contexts; 0: one list for all
    int N, nchunks;
    int64_t units;
    const float* blocks;
    int64_t block_floats;
    const float *b0, *W1, *b1, *W2, *b2, *W3, *b3;
    const float *cw, *cb, *wd, *bd;
    const float *d1_w, *d1_b, *d2_w, *d2_b, *att_W, *att_b, *lin_w, *lin_b, *bias;
    float* scores;
    int64_t row_stride;
    // the swept fields, sorted as in SweepCtxArgs; sweep_field(perm, a) = the caller's tuple column that holds the id of field f_a;
    // W0: the layer-0 filter (its swept-swept pairs)
    int nf;
    uint32_t fields, swept, perm;
    const float* W0;
};

// pairs with at least one of nf swept fields / with both
__host__ __device__ inline int sweep_live_pairs(int F, int nf) { return F * (F - 1) / 2 - (F - nf) * (F - nf - 1) / 2; }
__host__ __device__ inline int sweep_cross_pairs(int nf) { return nf * (nf - 1) / 2; }
// LDS of the candidate role for nf swept fields, in floats: C_0 | W_1 (padded image of conv_fwd_taps_body) | red | C_1 | C_2 | C_3 |
// U | V | small | rows | the layer-0 filter slices of the swept-swept pairs.  This one formula sizes the launch and answers
// cffm_sweep_ok (nf = 1) and cffm_sweep_tuples_ok.  Bytes at (Pp, K, nf), F the largest of that Pp: (48, 32, 1) 134,656; (48, 32, 2)
// 149,184; (48, 64, 2) 152,640; (48, 32, 3) 164,160 (832 over CFFM_LDS_WHOLE_CU: not served, nor is F = 9 at 163,648); (32, 32, 4)
// 113,216; (16, 32, 4) 54,848.
struct SweepLds { int C0, W1, red, C1, C2, C3, U, V, t1s, hpart, s0fix, A, fbrow, sc, wpart, lutf, aW, eo, Eall, wdp, Wx, floats; };
__host__ __device__ inline SweepLds sweep_lds(int Pp, int F, int K, int nf) {
    SweepLds l;
    int o = 0;
    l.C0 = o; o += 256 * Pp;                 // layers 2 and 3 reuse it for their 8 wave partials (2048 * NT floats)
    l.W1 = o; o += 4 * Pp * (Pp + 4);
    l.red = o; o += 64 * Pp;                 // layer 1: the partials of taps 2, 3 ([4 row tiles][NT][64 lanes] x 4); before the
                                             // candidate loop: the pair indices of the live pairs while wdp is staged
    l.C1 = o; o += 64 * Pp;
    l.C2 = o; o += 16 * Pp;
    l.C3 = o; o += 4 * Pp;
    l.U = o; o += nf * 2 * SWEEP_S * Pp;     // [a][dw][y][q]
    l.V = o; o += nf * 2 * SWEEP_S * Pp;     // [a][dh][x][q]
    l.t1s = o; o += 64;
    l.hpart = o; o += 8 * CFFM_HEAD_UNITS;
    l.s0fix = o; o += SWEEP_D;
    l.A = o; o += nf * SWEEP_D;
    l.fbrow = o; o += 16;                    // feature_bias by field: the context's, the candidate's at the swept slots
    l.sc = o; o += 16;                       // [1] first-order term, [3] fixed inner sum, [4 + a] R_a
    l.wpart = o; o += 16;
    l.lutf = o; o += nf > 1 ? 64 : 16;       // the live pairs (i | j << 16): at most 9 for one field, 30 for tuples (F = 10, nf = 4).
                                             // The served domain sits on these sizes: one field reaches K = 408 at F = 10 with 96 B left
    l.aW = o; o += 128;                      // att_W [F][F], F <= 10
    l.eo = o; o += nf * SWEEP_D;             // the candidate's outer rows, by sorted field
    l.Eall = o; o += F * K;                  // the context's inner rows with the candidate's rows at the swept fields
    l.wdp = o; o += sweep_live_pairs(F, nf) * K;     // dense(1) weights of the live pairs, in pair order
    l.Wx = o; o += sweep_cross_pairs(nf) * 4 * Pp;   // [pair (a < b)][dh][dw][q]
    l.floats = o;
    return l;
}

// This wave's share of conv layer l >= 1 on LDS-resident activations: row tile rt, filter tap `tap`, the channels 4 kk + t of
// every 16-channel block for t in [t0, t0 + tn) (the A / B fragment order of conv_fwd_taps_body).  Wt: this tap's [PP][PP]
// filter, `padded`: the LDS image with 16 floats behind every four rows.  Rows beyond the layer's So * So are clamped (their
// results are never stored).  Called under wave-uniform conditions only.
template <int NT>
__device__ __forceinline__ void sweep_conv_part(f32x4 (&acc)[NT], const float* inL, int lgSo, int rt, int tap, const float* Wt,
                                                bool padded, int t0, int tn, int act) {
    constexpr int PP = NT * 16;
    const int lane = threadIdx.x & 63, r = lane & 15, kk = lane >> 4;
    const int So = 1 << lgSo, Sin = 2 * So, rows = So * So;
    int m = rt * 16 + r;
    if (m >= rows) m = rows - 1;
    const int y = m >> lgSo, x = m & (So - 1), dh = tap >> 1, dw = tap & 1;
    const float* src = inL + ((2 * y + dh) * Sin + 2 * x + dw) * PP + 4 * kk;
#pragma unroll
    for (int h = 0; h < NT; ++h) {
        const float4 v = *reinterpret_cast<const float4*>(src + 16 * h);
        const float av[4] = {act_pos(v.x, act), act_pos(v.y, act), act_pos(v.z, act), act_pos(v.w, act)};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < t0 || t >= t0 + tn) continue;                // wave-uniform
            const int krow = 16 * h + 4 * kk + t;
            const float* wr = Wt + krow * PP + (padded ? (krow >> 2) * 16 : 0) + r;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma16(av[t], wr[nt * 16], acc[nt]);
        }
    }
}

// The same share for layers 2 and 3 (one row tile; tap = wave & 3, th = wave >> 2: the channels 4 kk + 2 th, 4 kk + 2 th + 1 of
// every 16-channel block) with this lane's B fragments in registers: w[h][tt][nt] = W[tap][16 h + 4 kk + 2 th + tt][16 nt + r].  They
// depend on the wave and the lane alone, so sweep_cand_kernel loads them once per launch (sweep_load_w).
template <int NT>
__device__ __forceinline__ void sweep_load_w(float (&w)[NT][2][NT], const float* W) {
    constexpr int PP = NT * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kk = lane >> 4, tap = wave & 3, th = wave >> 2;
#pragma unroll
    for (int h = 0; h < NT; ++h)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) w[h][tt][nt] = W[(tap * PP + 16 * h + 4 * kk + 2 * th + tt) * PP + nt * 16 + r];
}
template <int NT>
__device__ __forceinline__ void sweep_conv_part_reg(f32x4 (&acc)[NT], const float* inL, int lgSo, const float (&w)[NT][2][NT], int act) {
    constexpr int PP = NT * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kk = lane >> 4, tap = wave & 3, th = wave >> 2;
    const int So = 1 << lgSo, Sin = 2 * So, rows = So * So;
    const int m = r < rows ? r : rows - 1;
    const int y = m >> lgSo, x = m & (So - 1), dh = tap >> 1, dw = tap & 1;
    const float* src = inL + ((2 * y + dh) * Sin + 2 * x + dw) * PP + 4 * kk;
#pragma unroll
    for (int h = 0; h < NT; ++h) {
        const float4 v = *reinterpret_cast<const float4*>(src + 16 * h);
        const float a0 = act_pos(th ? v.z : v.x, act), a1 = act_pos(th ? v.w : v.y, act);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma16(a0, w[h][0][nt], acc[nt]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma16(a1, w[h][1][nt], acc[nt]);
    }
}

// s[off + y] = sum_{x,q} act(C[y][x][q]) for the S rows of one conv output in LDS (wave w takes rows w, w + 8, ...)
__device__ __forceinline__ void sweep_pool(const float* C, int S, int Pp, float* t1s, int off, int act) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n4 = S * Pp / 4;
    for (int y = wave; y < S; y += SWEEP_NTH / 64) {
        const float4* row = reinterpret_cast<const float4*>(C) + y * n4;
        float s = 0.f;
        for (int i = lane; i < n4; i += 64) {
            const float4 v = row[i];
            s += (act_pos(v.x, act) + act_pos(v.y, act)) + (act_pos(v.z, act) + act_pos(v.w, act));
        }
        s = wave_sum(s);
        if (lane == 0) t1s[off + y] = s;
    }
}

// layers 2 and 3: add the 8 wave partials in wave order, + bias, relu, rows < `rows` -> out [rows][PP]
template <int NT>
__device__ __forceinline__ void sweep_conv_reduce(const float* red2, const float* bias, float* out, int rows) {
    constexpr int PP = NT * 16;
    const int tid = threadIdx.x;
    if (tid < NT * 64) {
        const int nt = tid >> 6, ln = tid & 63;
        const f32x4* p = reinterpret_cast<const f32x4*>(red2);
        f32x4 v = p[nt * 64 + ln];
#pragma unroll
        for (int w = 1; w < SWEEP_NTH / 64; ++w) v += p[(w * NT + nt) * 64 + ln];
        const int n = nt * 16 + (ln & 15);
        const float bv = bias[n];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = (ln >> 4) * 4 + j;
            if (m < rows) out[m * PP + n] = fmaxf(v[j] + bv, 0.f);
        }
    }
}

// NF: the number of swept fields as a compile-time constant (1: cffm_score_sweep / _lists, and tuples of one); 0: a.nf, 2 ..
// CFFM_SWEEP_MAX_NF.  The body is one code for every nf; at NF = 1 its loops over the swept fields unroll and the loop over the
// swept-swept pairs is empty.
template <int NT, int NF>
__global__ __launch_bounds__(SWEEP_NTH) void sweep_cand_kernel(SweepArgs a) {
    constexpr int PP = NT * 16, PQ = PP / 4, NTH = SWEEP_NTH, NWV = NTH / 64, D = SWEEP_D, S = SWEEP_S;
    constexpr int ZR = S * S * PQ / NTH;                         // float4 of Zctx per thread: 2 * NT
    static_assert(ZR * NTH == S * S * PQ, "Zctx divides evenly over the workgroup");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Geo& g = a.g;
    const int F = g.F, K = g.K, act = g.act, K4 = K / 4, K2 = K / 2;
    const int nf = NF ? NF : a.nf;
    const SweepLds L = sweep_lds(PP, F, K, nf);
    const SweepBlock bo = sweep_block(PP, F, K, nf);
    float* sm = reinterpret_cast<float*>(smem);
    float *C0 = sm + L.C0, *W1s = sm + L.W1, *red = sm + L.red, *C1 = sm + L.C1, *C2 = sm + L.C2, *C3 = sm + L.C3;
    float *Us = sm + L.U, *Vs = sm + L.V, *t1s = sm + L.t1s, *s0fix = sm + L.s0fix, *As = sm + L.A, *fbrow = sm + L.fbrow;
    float *sc = sm + L.sc, *wpart = sm + L.wpart, *aW = sm + L.aW, *eo = sm + L.eo, *Eall = sm + L.Eall, *wdp = sm + L.wdp;
    float (*hpart)[CFFM_HEAD_UNITS] = reinterpret_cast<float (*)[CFFM_HEAD_UNITS]>(sm + L.hpart);
    uint32_t* lutf = reinterpret_cast<uint32_t*>(sm + L.lutf);
    float* red2 = C0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kk = lane >> 4;

    // ---- once per workgroup: what depends on (theta, field) alone ----
    for (int i = tid; i < 4 * PP * PQ; i += NTH) {               // W_1 -> the padded image: row k of a tap at k * PP + (k >> 2) * 16
        const int row = i / PQ, c4 = i - row * PQ, tap = row / PP, krow = row - tap * PP;
        *reinterpret_cast<float4*>(W1s + tap * PP * (PP + 4) + krow * PP + (krow >> 2) * 16 + 4 * c4) =
            reinterpret_cast<const float4*>(a.W1)[i];
    }
    {
        // the live pairs (at least one swept field) in pair order: pair p on lane p of wave 0 (P <= 45), compacted by ballot.  Their
        // pair indices are needed only until wdp is gathered: they borrow `red`, which layer 1 first writes inside the candidate loop.
        uint32_t* pidx = reinterpret_cast<uint32_t*>(red);
        if (wave == 0) {
            int i = 0, base = 0;
            while (i < F - 2 && lane >= base + F - 1 - i) { base += F - 1 - i; ++i; }
            const int j = lane < g.P ? i + 1 + lane - base : i;
            const bool live = lane < g.P && (((a.swept >> i) | (a.swept >> j)) & 1u);
            const unsigned long long m = __ballot(live);
            if (live) {
                const int q = __popcll(m & ((1ull << lane) - 1ull));
                lutf[q] = (uint32_t)i | ((uint32_t)j << 16);
                pidx[q] = (uint32_t)lane;
            }
        }
        __syncthreads();
        for (int i = tid; i < sweep_live_pairs(F, nf) * K; i += NTH) {
            const int q = i / K, c = i - q * K;
            wdp[i] = a.wd[(int64_t)pidx[q] * K + c];
        }
        // the layer-0 filter of the swept-swept pairs (f_a, f_b), a < b in that order: [dh][dw][q] each
        float* Wx = sm + L.Wx;
        int pr = 0;
        for (int sa = 0; sa < nf; ++sa)
            for (int sb = sa + 1; sb < nf; ++sb, ++pr) {
                const int prow = sweep_pair(sweep_field(a.fields, sa), sweep_field(a.fields, sb), F);
                for (int i = tid; i < 4 * PP; i += NTH) {
                    const int tap = i / PP, q = i - tap * PP;
                    Wx[pr * 4 * PP + i] = a.W0[(tap * PP + prow) * PP + q];
                }
            }
    }
    if (g.linear_att)
        for (int i = tid; i < F * F; i += NTH) aW[i] = a.att_W[i];
    const float cw[4] = {a.cw[0], a.cw[1], a.cw[2], a.cw[3]};
    const float cb[2] = {a.cb[0], a.cb[1]};
    // dense(32): 8 partial sums per unit on the first 256 threads (head_fwd_body), this thread's kernel rows in registers
    constexpr int T1W = 2 * D - 2, KPP = (T1W + 7) / 8;
    const int hq = tid & 31, hp = tid >> 5;
    float w1r[KPP];
#pragma unroll
    for (int i = 0; i < KPP; ++i) {
        const int k = hp * KPP + i;
        w1r[i] = (tid < 256 && k < T1W) ? a.d1_w[k * CFFM_HEAD_UNITS + hq] : 0.f;
    }
    float d1b = 0.f, d2w = 0.f, linw = 0.f, attb = 0.f;
    if (lane < CFFM_HEAD_UNITS) { d1b = a.d1_b[lane]; d2w = a.d2_w[lane]; }
    if (lane < F && g.linear_att) { linw = a.lin_w[lane]; attb = a.att_b[lane]; }
    const float d2b = a.d2_b[0], linb = g.linear_att ? a.lin_b[0] : 0.f, biasv = a.bias[0], bdv = a.bd[0];
    const int nun = sweep_live_pairs(F, nf) * K2;
    float w2r[NT][2][NT], w3r[NT][2][NT];                        // this lane's filter fragments of layers 2 and 3, for the whole launch
    sweep_load_w<NT>(w2r, a.W2);
    sweep_load_w<NT>(w3r, a.W3);

    // this thread's piece of a candidate's rows: per swept field K/4 inner pieces, D/4 outer pieces and one feature_bias value, field
    // f_a's on threads [a * per, (a + 1) * per) (one field: slot 0 without the division, a constant for the compiler)
    const int32_t* cand = a.cand;                                // the current unit's list
    const int per = K4 + D / 4 + 1, fa_slot = nf > 1 ? tid / per : 0, fa_piece = tid - fa_slot * per;
    auto fetch = [&](int n) -> float4 {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < nf * per) {
            const int id = sweep_clamp(cand[(int64_t)n * nf + sweep_field(a.perm, fa_slot)], g.M);
            if (fa_piece < K4) v = reinterpret_cast<const float4*>(a.inner)[(int64_t)id * K4 + fa_piece];
            else if (fa_piece < K4 + D / 4) v = reinterpret_cast<const float4*>(a.outer)[(int64_t)id * (D / 4) + fa_piece - K4];
            else v.x = a.fbias[id];
        }
        return v;
    };
    auto put = [&](const float4& v) {
        if (tid < nf * per) {
            const int fa = sweep_field(a.fields, fa_slot);
            if (fa_piece < K4) reinterpret_cast<float4*>(Eall + fa * K)[fa_piece] = v;
            else if (fa_piece < K4 + D / 4) reinterpret_cast<float4*>(eo + fa_slot * D)[fa_piece - K4] = v;
            else fbrow[fa] = v.x;
        }
    };

    for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int64_t c = u / a.nchunks;
        const int64_t first = (u - c * a.nchunks) * CFFM_SWEEP_CHUNK;        // 64 bits: N may lie within a chunk of 2^31
        const int n0 = (int)first;
        const int n1 = first + CFFM_SWEEP_CHUNK < a.N ? n0 + CFFM_SWEEP_CHUNK : a.N;
        const float* blk = a.blocks + c * a.block_floats;
        cand = a.cand + c * a.cand_ctx_stride;
        __syncthreads();
        // ---- stage the context's block: Zctx + b in registers, the rest in LDS ----
        float4 Zr[ZR];
#pragma unroll
        for (int k = 0; k < ZR; ++k) {
            const int i4 = tid + NTH * k;
            const float4 z = reinterpret_cast<const float4*>(blk + bo.Z)[i4];
            const float4 b = reinterpret_cast<const float4*>(a.b0)[i4 % PQ];
            Zr[k] = make_float4(z.x + b.x, z.y + b.y, z.z + b.z, z.w + b.w);
        }
        for (int i = tid; i < nf * 2 * S * PQ; i += NTH) {
            reinterpret_cast<float4*>(Us)[i] = reinterpret_cast<const float4*>(blk + bo.U)[i];
            reinterpret_cast<float4*>(Vs)[i] = reinterpret_cast<const float4*>(blk + bo.V)[i];
        }
        // the swept rows and slots are the candidate's: put() writes them
        for (int i = tid; i < F * K4; i += NTH)
            if (!((a.swept >> (i / K4)) & 1u)) reinterpret_cast<float4*>(Eall)[i] = reinterpret_cast<const float4*>(blk + bo.Ei)[i];
        if (tid < D) s0fix[tid] = blk[bo.s0fix + tid];
        if (tid < nf * D) As[tid] = blk[bo.A + tid];
        if (tid < 16 && !((a.swept >> tid) & 1u)) fbrow[tid] = blk[bo.fb + tid];
        if (tid < 1 + nf) sc[3 + tid] = blk[bo.scal + tid];
        float4 pre = fetch(n0);
        put(pre);
        __syncthreads();

        for (int n = n0; n < n1; ++n) {
            const bool more = n + 1 < n1;
            if (more) pre = fetch(n + 1);                        // in flight across this candidate's arithmetic
            // ---- phase 1: C_0 = relu(Z); the candidate's inner pairs; s0; the first-order term ----
#pragma unroll
            for (int k = 0; k < ZR; ++k) {
                const int i4 = tid + NTH * k, q4 = i4 % PQ, pix = i4 / PQ, y = pix >> 4, x = pix & 15;
                // z += p0 * w0 + p1 * w1 + p2 * w2 + p3 * w3, four multiply-adds per channel in this order
                auto fma4 = [](float4& z, float p0, const float4& w0, float p1, const float4& w1, float p2, const float4& w2, float p3,
                               const float4& w3) {
                    z.x = fmaf(p3, w3.x, fmaf(p2, w2.x, fmaf(p1, w1.x, fmaf(p0, w0.x, z.x))));
                    z.y = fmaf(p3, w3.y, fmaf(p2, w2.y, fmaf(p1, w1.y, fmaf(p0, w0.y, z.y))));
                    z.z = fmaf(p3, w3.z, fmaf(p2, w2.z, fmaf(p1, w1.z, fmaf(p0, w0.z, z.z))));
                    z.w = fmaf(p3, w3.w, fmaf(p2, w2.w, fmaf(p1, w1.w, fmaf(p0, w0.w, z.w))));
                };
                // per swept field, in sorted order: e_a[2x+dw] * U_a[dw][y], then e_a[2y+dh] * V_a[dh][x]
                float4 z = Zr[k];
                for (int sa = 0; sa < nf; ++sa) {
                    const float* ea = eo + sa * D;
                    const float ex0 = ea[2 * x], ex1 = ea[2 * x + 1], ey0 = ea[2 * y], ey1 = ea[2 * y + 1];
                    // (the spelling of these four addresses decides the register count of the single-field instances: this one
                    // keeps all six at or below what they took with a path of their own, profiles/sweep_one_path.md)
                    const int iv = (2 * sa * S + x) * PQ + q4;
                    fma4(z, ex0, reinterpret_cast<const float4*>(Us)[((2 * sa) * S + y) * PQ + q4], ex1,
                         reinterpret_cast<const float4*>(Us)[((2 * sa + 1) * S + y) * PQ + q4], ey0, reinterpret_cast<const float4*>(Vs)[iv],
                         ey1, reinterpret_cast<const float4*>(Vs)[iv + S * PQ]);
                }
                // then the swept-swept pairs (a < b), each X_ab = sum_dh sum_dw (e_a[2y+dh] * e_b[2x+dw]) * W[dh][dw][(f_a, f_b)]
                const float4* wx = reinterpret_cast<const float4*>(sm + L.Wx) + q4;
                for (int sa = 0; sa < nf; ++sa)
                    for (int sb = sa + 1; sb < nf; ++sb, wx += 4 * PQ) {
                        const float *ea = eo + sa * D, *eb = eo + sb * D;
                        fma4(z, ea[2 * y] * eb[2 * x], wx[0], ea[2 * y] * eb[2 * x + 1], wx[PQ], ea[2 * y + 1] * eb[2 * x], wx[2 * PQ],
                             ea[2 * y + 1] * eb[2 * x + 1], wx[3 * PQ]);
                    }
                reinterpret_cast<float4*>(C0)[i4] = make_float4(fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f));
            }
            {
                float part = 0.f;
                for (int q = tid; q < nun; q += NTH) {
                    const int sl = q / K2, t = q - sl * K2;
                    const InnerUnit v = inner_unit(Eall, lutf, sl, t, K, cw, cb, act);
                    const float2 w2 = *reinterpret_cast<const float2*>(&wdp[sl * K + 2 * t]);
                    part += v.s0 * w2.x + v.s1 * w2.y;
                }
                part = wave_sum(part);
                if (lane == 0) wpart[wave] = part;
            }
            if (wave == 0) {             // s0[h] = s0fix[h] + sum_a (A_a[h] * rowsum(e_a) + e_a[h] * R_a) + sum_{a<b} e_a[h] * rowsum(e_b),
                                         // one term at a time onto s, per field in sorted order: A_a, R_a, then the fields below a
                float s = lane < D ? s0fix[lane] : 0.f, below = 0.f;                 // below: sum of e_a'[h] over a' < a
#pragma nounroll                         // a run-time nf keeps one loop body (peeling a = 0 off cost the kernel two VGPRs)
                for (int sa = 0; sa < nf; ++sa) {
                    const float ev = lane < D ? eo[sa * D + lane] : 0.f;
                    const float rse = wave_sum(ev);
                    s = s + (lane < D ? As[sa * D + lane] : 0.f) * rse;
                    s = s + ev * sc[4 + sa];
                    if (sa > 0) s = s + below * rse;
                    below += ev;
                }
                if (lane < D) t1s[lane] = s;
            }
            if (wave == NWV - 1) {                               // first-order term (head_fwd_body), CFFM.py:422-446
                const float fbv = lane < F ? fbrow[lane] : 0.f;
                float lin;
                if (g.linear_att) {
                    float z = attb;
                    for (int gI = 0; gI < F; ++gI) {
                        const float fg = __shfl(fbv, gI, 64);
                        if (lane < F) z += fg * aW[gI * F + lane];
                    }
                    z = lane < F ? z / g.lamda_att : -INFINITY;
                    const float mx = wave_max(z);
                    const float e = lane < F ? expf(z - mx) : 0.f;
                    const float den = wave_sum(e);
                    lin = wave_sum(lane < F ? fbv * (e / den) * linw : 0.f) + linb;
                } else {
                    lin = wave_sum(fbv);
                }
                if (lane == 0) sc[1] = lin;
            }
            lds_barrier();
            // ---- phase 2: pool of C_0; layer 1: wave w takes row tile w & 3 and the taps 2 (w >> 2), 2 (w >> 2) + 1 ----
            sweep_pool(C0, S, PP, t1s, D, act);
            f32x4 acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            {
                const int rt = wave & 3, kh = wave >> 2;
                sweep_conv_part<NT>(acc, C0, 3, rt, 2 * kh, W1s + (2 * kh) * PP * (PP + 4), true, 0, 4, act);
                sweep_conv_part<NT>(acc, C0, 3, rt, 2 * kh + 1, W1s + (2 * kh + 1) * PP * (PP + 4), true, 0, 4, act);
                if (kh == 1) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) reinterpret_cast<f32x4*>(red)[(rt * NT + nt) * 64 + lane] = acc[nt];
                }
            }
            lds_barrier();
            if (wave < 4) {                                      // taps 0, 1 + taps 2, 3, + bias, relu -> C_1
                const int rt = wave;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const f32x4 o = reinterpret_cast<const f32x4*>(red)[(rt * NT + nt) * 64 + lane];
                    const float bv = a.b1[nt * 16 + r];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        C1[(rt * 16 + kk * 4 + j) * PP + nt * 16 + r] = fmaxf((acc[nt][j] + o[j]) + bv, 0.f);
                }
            }
            lds_barrier();
            // ---- layers 2 and 3: one row tile; wave w takes tap w & 3 and two of the four channels of every fragment ----
            sweep_pool(C1, 8, PP, t1s, D + 16, act);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            sweep_conv_part_reg<NT>(acc, C1, 2, w2r, act);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) reinterpret_cast<f32x4*>(red2)[(wave * NT + nt) * 64 + lane] = acc[nt];
            lds_barrier();
            sweep_conv_reduce<NT>(red2, a.b2, C2, 16);
            lds_barrier();
            sweep_pool(C2, 4, PP, t1s, D + 24, act);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            sweep_conv_part_reg<NT>(acc, C2, 1, w3r, act);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) reinterpret_cast<f32x4*>(red2)[(wave * NT + nt) * 64 + lane] = acc[nt];
            lds_barrier();
            sweep_conv_reduce<NT>(red2, a.b3, C3, 4);
            lds_barrier();
            sweep_pool(C3, 2, PP, t1s, D + 28, act);
            lds_barrier();
            // ---- dense(32), dense(1) * beta, add_n (CFFM.py:409-414, :449-453) ----
            if (tid < 256) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < KPP; ++i) {
                    const int k = hp * KPP + i;
                    if (k < T1W) s += t1s[k] * w1r[i];
                }
                hpart[hp][hq] = s;
            }
            lds_barrier();
            if (wave == 0) {
                float h = 0.f;
                if (lane < CFFM_HEAD_UNITS) {
                    h = d1b;
#pragma unroll
                    for (int pp = 0; pp < 8; ++pp) h += hpart[pp][lane];
                }
                const float v = wave_sum(lane < CFFM_HEAD_UNITS ? h * d2w : 0.f);
                if (lane == 0) {
                    float io = sc[3];
#pragma unroll
                    for (int w = 0; w < NWV; ++w) io += wpart[w];
                    float out = io + bdv;
                    out += g.beta_outer * (v + d2b);
                    out += sc[1];
                    out += biasv;
                    if (a.loss == CFFM_LOSS_LOG) out = 1.f / (1.f + expf(-out));     // what cffm_predict returns for log_loss
                    a.scores[c * a.row_stride + n] = out;
                }
            }
            if (more) put(pre);
            lds_barrier();
        }
    }
}

// LDS of the candidate role for nf swept fields, in bytes: what the launcher asks for and what the served-domain queries compare
static inline size_t sweep_cand_lds(int Pp, int F, int K, int nf) { return (size_t)sweep_lds(Pp, F, K, nf).floats * 4; }

template <int NT, int NF>
int sweep_launch(const SweepCtxArgs& ca, const SweepArgs& sa, int C, int grid, hipStream_t st) {
    const Geo& g = sa.g;
    const size_t lds_c = sweep_ctx_lds(g.Pp, g.F, g.K), lds_k = sweep_cand_lds(g.Pp, g.F, g.K, sa.nf);
    int rc = set_lds(sweep_ctx_kernel<NT>, lds_c);
    if (rc) return rc;
    rc = set_lds(sweep_cand_kernel<NT, NF>, lds_k);
    if (rc) return rc;
    hipLaunchKernelGGL(sweep_ctx_kernel<NT>, dim3((unsigned)C), dim3(256), lds_c, st, ca);
    CFFM_CHECK_LAUNCH();
    hipLaunchKernelGGL((sweep_cand_kernel<NT, NF>), dim3((unsigned)grid), dim3(SWEEP_NTH), lds_k, st, sa);
    CFFM_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int cffm_sweep_ok(const cffm_shape_t* s) {
    if (check_shape(s)) return 0;
    const Geo g = make_geo(s);
    if (!s->inner_conv || !s->outer_conv || s->D != SWEEP_D || g.Pp > SWEEP_MAXPP) return 0;
    if (check_lds(s)) return 0;
    if (s->K / 4 + SWEEP_D / 4 + 1 > SWEEP_NTH) return 0;                          // a candidate's rows: one piece per thread
    if (sweep_ctx_lds(g.Pp, g.F, g.K) > (size_t)CFFM_LDS_WHOLE_CU) return 0;
    if (sweep_cand_lds(g.Pp, g.F, g.K, 1) > (size_t)CFFM_LDS_WHOLE_CU) return 0;
    return 1;
}

extern "C" int cffm_sweep_tuples_ok(const cffm_shape_t* s, int32_t nf) {
    if (!cffm_sweep_ok(s) || nf < 1 || nf > CFFM_SWEEP_MAX_NF || nf > s->F) return 0;
    const Geo g = make_geo(s);
    if (nf * (s->K / 4 + SWEEP_D / 4 + 1) > SWEEP_NTH) return 0;                   // a candidate's rows: one piece per thread
    return sweep_cand_lds(g.Pp, g.F, g.K, nf) <= (size_t)CFFM_LDS_WHOLE_CU;
}

extern "C" int64_t cffm_sweep_tuples_scratch_bytes(const cffm_shape_t* s, int32_t nf, int32_t C) {
    if (C < 0 || !cffm_sweep_tuples_ok(s, nf)) return -1;
    const Geo g = make_geo(s);
    return SWEEP_HEADER + (int64_t)C * sweep_block(g.Pp, g.F, g.K, nf).floats * 4;
}

extern "C" int64_t cffm_sweep_scratch_bytes(const cffm_shape_t* s, int32_t C) { return cffm_sweep_tuples_scratch_bytes(s, 1, C); }

// The block layout for nf swept fields into *t.  `out` is the caller's pointer, looked at only for the refusal, in the documented order.
static int sweep_layout(const cffm_shape_t* s, int32_t nf, const void* out, cffm_sweep_tuples_block_t* t) {
    int rc = check_shape(s);
    if (rc) return rc;
    if (!out) return CFFM_ERR_BAD_SHAPE;
    if (!cffm_sweep_tuples_ok(s, nf)) return CFFM_ERR_UNSUPPORTED;
    const Geo g = make_geo(s);
    const SweepBlock b = sweep_block(g.Pp, g.F, g.K, nf);
    t->header_floats = SWEEP_HEADER / 4;
    t->block_floats = b.floats;
    t->Z = b.Z; t->U = b.U; t->V = b.V; t->Ei = b.Ei;
    t->s0fix = b.s0fix; t->A = b.A; t->fb = b.fb; t->scal = b.scal;
    t->UV_stride = 2 * SWEEP_S * g.Pp;
    t->A_stride = SWEEP_D;
    return 0;
}

extern "C" int cffm_sweep_tuples_block_layout(const cffm_shape_t* s, int32_t nf, cffm_sweep_tuples_block_t* out) {
    return sweep_layout(s, nf, out, out);
}

// the nf = 1 answer without the two stride members, which end the tuples' struct
static_assert(offsetof(cffm_sweep_tuples_block_t, UV_stride) == sizeof(cffm_sweep_block_t), "cffm_sweep_block_t is a prefix");
extern "C" int cffm_sweep_block_layout(const cffm_shape_t* s, cffm_sweep_block_t* out) {
    cffm_sweep_tuples_block_t t;
    const int rc = sweep_layout(s, 1, out, &t);
    if (rc == 0) memcpy(out, &t, sizeof *out);
    return rc;
}

// The two launches for nf swept fields, sorted: fields[a] = f_a, col[a] = the caller's tuple column of f_a.  Every argument has been
// checked by the caller.
static int sweep_run(const cffm_shape_t* s, const cffm_tables_t* tab, const float* theta, const int32_t* ctx, int32_t C, int nf,
                     const int* fields, const int* col, const int32_t* cand, int64_t cand_ctx_stride, int32_t N, float* scores,
                     int64_t row_stride, void* scratch, void* stream) {
    const Geo g = make_geo(s);
    cffm_theta_layout_t tl;
    int rc = cffm_theta_layout(s, &tl);
    if (rc) return rc;
    const SweepBlock bo = sweep_block(g.Pp, g.F, g.K, nf);
    float* blocks = reinterpret_cast<float*>((char*)scratch + SWEEP_HEADER);
    uint32_t packed = 0, swept = 0, perm = 0;
    for (int a = 0; a < nf; ++a) {
        packed |= (uint32_t)fields[a] << (4 * a);
        perm |= (uint32_t)col[a] << (4 * a);
        swept |= 1u << fields[a];
    }
    SweepCtxArgs ca;
    ca.g = g;
    ca.inner = tab->inner_emb; ca.outer = tab->outer_emb; ca.fbias = tab->feat_bias;
    ca.ctx = ctx; ca.nf = nf; ca.fields = packed; ca.swept = swept;
    ca.W0 = theta + tl.conv_w[0]; ca.cw = theta + tl.inner_cw; ca.cb = theta + tl.inner_cb; ca.wd = theta + tl.inner_dw;
    ca.blocks = blocks; ca.block_floats = bo.floats;
    SweepArgs sa;
    sa.g = g; sa.loss = s->loss;
    sa.inner = tab->inner_emb; sa.outer = tab->outer_emb; sa.fbias = tab->feat_bias;
    sa.cand = cand; sa.cand_ctx_stride = cand_ctx_stride; sa.N = N;
    sa.nf = nf; sa.fields = packed; sa.swept = swept; sa.perm = perm;
    sa.nchunks = (int)(((int64_t)N + CFFM_SWEEP_CHUNK - 1) / CFFM_SWEEP_CHUNK);
    sa.units = (int64_t)C * sa.nchunks;
    sa.blocks = blocks; sa.block_floats = bo.floats;
    sa.W0 = ca.W0; sa.b0 = theta + tl.conv_b[0];
    sa.W1 = theta + tl.conv_w[1]; sa.b1 = theta + tl.conv_b[1];
    sa.W2 = theta + tl.conv_w[2]; sa.b2 = theta + tl.conv_b[2];
    sa.W3 = theta + tl.conv_w[3]; sa.b3 = theta + tl.conv_b[3];
    sa.cw = ca.cw; sa.cb = ca.cb; sa.wd = ca.wd; sa.bd = theta + tl.inner_db;
    sa.d1_w = theta + tl.d1_w; sa.d1_b = theta + tl.d1_b; sa.d2_w = theta + tl.d2_w; sa.d2_b = theta + tl.d2_b;
    sa.att_W = theta + tl.att_W; sa.att_b = theta + tl.att_b; sa.lin_w = theta + tl.lin_w; sa.lin_b = theta + tl.lin_b;
    sa.bias = theta + tl.bias;
    sa.scores = scores; sa.row_stride = row_stride;
    // one 512-thread workgroup fits a CU (130 KB of LDS at Pp = 48): two per CU of the chip's 256 keep the tail of the static
    // unit loop short without staging W_1 more often than that
    const int64_t max_grid = 512;
    const int grid = (int)(sa.units < max_grid ? sa.units : max_grid);
    hipStream_t st = (hipStream_t)stream;
    switch (g.Pp / 16 * 2 + (nf > 1)) {                          // one field: the count compiled in; tuples: a.nf
        case 2: return sweep_launch<1, 1>(ca, sa, C, grid, st);
        case 3: return sweep_launch<1, 0>(ca, sa, C, grid, st);
        case 4: return sweep_launch<2, 1>(ca, sa, C, grid, st);
        case 5: return sweep_launch<2, 0>(ca, sa, C, grid, st);
        case 6: return sweep_launch<3, 1>(ca, sa, C, grid, st);
        case 7: return sweep_launch<3, 0>(ca, sa, C, grid, st);
        default: return CFFM_ERR_UNSUPPORTED;
    }
}

// The one checked entry: cffm_score_sweep_tuples.  Its refusals, in the order include/cffm_hip.h documents; for one field they are those
// of cffm_score_sweep / _lists in theirs (cffm_sweep_tuples_ok(s, 1) == cffm_sweep_ok(s), and what lies between is CFFM_ERR_BAD_SHAPE).
extern "C" int cffm_score_sweep_tuples(const cffm_shape_t* s, const cffm_tables_t* tab, const float* theta, const int32_t* ctx, int32_t C,
                                       const int32_t* fields, int32_t nf, const int32_t* cand, int64_t cand_ctx_stride, int32_t N,
                                       float* scores, int64_t row_stride, void* scratch, void* stream) {
    int rc = check_shape(s);
    if (rc) return rc;
    if (!cffm_sweep_ok(s)) return CFFM_ERR_UNSUPPORTED;
    if (nf < 1 || nf > s->F || !fields) return CFFM_ERR_BAD_SHAPE;
    int sorted[CFFM_MAX_FIELDS], col[CFFM_MAX_FIELDS], slot[CFFM_MAX_FIELDS];
    for (int f = 0; f < s->F; ++f) slot[f] = -1;
    for (int a = 0; a < nf; ++a) {
        const int f = fields[a];
        if (f < 0 || f >= s->F || slot[f] >= 0) return CFFM_ERR_BAD_SHAPE;         // outside [0, F), or the same field twice
        slot[f] = a;
    }
    if (!cffm_sweep_tuples_ok(s, nf)) return CFFM_ERR_UNSUPPORTED;
    if (N < 1 || C < 0 || row_stride < N) return CFFM_ERR_BAD_SHAPE;
    if (cand_ctx_stride < 0 || (cand_ctx_stride != 0 && cand_ctx_stride < (int64_t)N * nf)) return CFFM_ERR_BAD_SHAPE;
    if (C == 0) return 0;
    if (!tab || !tab->inner_emb || !tab->outer_emb || !tab->feat_bias || !theta || !ctx || !cand || !scores || !scratch)
        return CFFM_ERR_BAD_SHAPE;
    int n = 0;
    for (int f = 0; f < s->F; ++f)                                                 // by field: the caller's order ends here
        if (slot[f] >= 0) { sorted[n] = f; col[n] = slot[f]; ++n; }
    return sweep_run(s, tab, theta, ctx, C, nf, sorted, col, cand, cand_ctx_stride, N, scores, row_stride, scratch, stream);
}

extern "C" int cffm_score_sweep(const cffm_shape_t* s, const cffm_tables_t* tab, const float* theta, const int32_t* ctx, int32_t C,
                                int32_t field, const int32_t* cand, int32_t N, float* scores, int64_t row_stride, void* scratch,
                                void* stream) {
    return cffm_score_sweep_tuples(s, tab, theta, ctx, C, &field, 1, cand, 0, N, scores, row_stride, scratch, stream);
}

extern "C" int cffm_score_sweep_lists(const cffm_shape_t* s, const cffm_tables_t* tab, const float* theta, const int32_t* ctx, int32_t C,
                                      int32_t field, const int32_t* cand, int64_t cand_ctx_stride, int32_t N, float* scores,
                                      int64_t row_stride, void* scratch, void* stream) {
    return cffm_score_sweep_tuples(s, tab, theta, ctx, C, &field, 1, cand, cand_ctx_stride, N, scores, row_stride, scratch, stream);
}

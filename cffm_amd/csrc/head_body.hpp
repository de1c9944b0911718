// Device body of the head forward (shared by head_fwd_kernel and the fused forward kernel).
#pragma once
#include "common.hpp"

struct HeadArgs {
    Geo g;
    int B;
    const float* Eo;          // [B,F,D]
    const float* fb;          // [B,F]
    const float* inner_out;   // [B]
    const float* C[CFFM_MAX_LAYERS];
    const float *d1_w, *d1_b, *d2_w, *d2_b, *att_W, *att_b, *lin_w, *lin_b, *bias;
    const float* y;           // may be NULL
    float *t1, *h1, *att, *out, *sqerr;
    int loss, inner_conv, outer_conv;
    int s0_ready = 0;         // 1: t1[b][0:D] already holds the s0 pool (cffm_gather_inner_fwd_wide wrote it) and Eo is not read
    const float* pool[CFFM_MAX_LAYERS] = {};   // wide shapes: partial sum pools left by the conv epilogues, [B][S_l][pool_np[l]]
    int pool_np[CFFM_MAX_LAYERS] = {};         // 0: sweep C_l here
};

__device__ __forceinline__ float loss_term(float out_raw, float y, int loss, float* out_eval) {
    switch (loss) {
        case CFFM_LOSS_MAE: *out_eval = out_raw; return fabsf(y - out_raw);
        case CFFM_LOSS_SQUARE_L2: *out_eval = out_raw; return 0.5f * (y - out_raw) * (y - out_raw);   // tf.nn.l2_loss
        case CFFM_LOSS_LOG: {
            const float s = 1.f / (1.f + expf(-out_raw));
            *out_eval = s;                                         // CFFM.py:496
            return -(y * logf(s + 1e-7f) + (1.f - y) * logf(1.f - s + 1e-7f));
        }
        default: *out_eval = out_raw; return (y - out_raw) * (y - out_raw);
    }
}

// One workgroup per example.  Everything that does not depend on an earlier phase is loaded first (the
// embedding tile, this thread's slice of the dense(32) kernel, the first-order inputs), so the kernel pays the
// L2/HBM latency once instead of once per phase; the pooling sweep keeps four rows in flight per lane.
#define HEAD_KPP 16      // preloaded dense(32) rows per thread: covers 2D-2 <= 128
// dynamic LDS: head_fwd_lds(g), common.hpp

// NW wavefronts: the pooling sweeps, the embedding tile and s0 use all of them; the dense(32) partials stay on the
// first 256 threads (8 parts x 32 units)
// CL (fused forward): LDS copies of this example's conv outputs (at fused_c_off(l, c0_off, c1_off, ..) inside smem) are read
// instead of the global ones
// POOLS: the stand-alone head of the wide shapes takes s0 and the layer pools as left by earlier kernels (s0_ready, pool[]).  The
// fused forward instantiates POOLS = false: a.pool[l] / a.pool_np[l] with a run-time l would be a dynamically indexed member of a
// by-value kernel argument, i.e. a private copy in scratch memory inside the single-launch forward (it cost fwd_all 1.4 us).
// F_ / D_ != 0 (compiled-shape fused forward): field count and outer row length as constants - `live`, the pool sizes, the F loops and
// the width of t1 fold
template <int NW = 4, int ACTC = -1, bool POOLS = false, int F_ = 0, int D_ = 0>
__device__ __forceinline__ void head_fwd_body(const HeadArgs& a, int b, char* smem, bool CL = false, int c0_off = 0, int c1_off = 0) {
    const int act = ACTC >= 0 ? ACTC : a.g.act;         // ACTC >= 0: compile-time activation id (README shapes)
    constexpr int NTH = 64 * NW, RPW = 16 / NW;                    // rows per wave in one pooling sweep
    float* t1s = reinterpret_cast<float*>(smem);                   // [1024]
    float (*hpart)[CFFM_HEAD_UNITS] = reinterpret_cast<float (*)[CFFM_HEAD_UNITS]>(t1s + 1024);   // [8][32]
    float* rs = t1s + 1024 + 8 * CFFM_HEAD_UNITS;                  // [CFFM_MAX_FIELDS]
    float* sc = rs + CFFM_MAX_FIELDS;                              // [4]
    float* Et = sc + 4;                                            // [F][D] embedding tile of this example
    const Geo& g = a.g;
    const int F = F_ ? F_ : g.F, D = D_ ? D_ : g.D, Pp = F_ ? (F_ * (F_ - 1) / 2 + 15) / 16 * 16 : g.Pp;
    int live = g.live;
    if (D_) { live = -1; for (int d = D_; d > 1; d >>= 1) ++live; }  // make_geo: live = log2(D) - 1
    float* aW = Et + F * D;                                        // [F][F] attention matrix, staged and used by one wave only
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t1w = 2 * D - 2;
    const int q = tid & 31, part = tid >> 5, kpp = (t1w + 7) / 8;
    PHASE_MARK3(0);
    // ---- phase 0: independent loads ------------------------------------------------------------------------
    float w1r[HEAD_KPP];
    const bool pre = a.outer_conv && kpp <= HEAD_KPP;
    if (pre && tid < 256) {
#pragma unroll
        for (int i = 0; i < HEAD_KPP; ++i) {
            const int k = part * kpp + i;
            w1r[i] = (i < kpp && k < t1w) ? a.d1_w[k * CFFM_HEAD_UNITS + q] : 0.f;
        }
    }
    // every scalar / per-lane parameter of the later phases is requested now, so that no phase waits on L2 again
    float fbv = 0.f, attb = 0.f, linw = 0.f, linb = 0.f, d1b = 0.f, d2w = 0.f, d2b = 0.f, io = 0.f, biasv = 0.f, yv = 0.f;
    // the first-order term runs on the LAST wavefront: the first ones carry the pooling rows of the small top layers, and
    // the barrier behind the pools waited 1.9 us for wave 1 when it did both (phase timers, frappe)
    constexpr int FO = NW - 1;
    if (wave == FO) {
        if (lane < F) {
            fbv = a.fb[(int64_t)b * F + lane];
            linw = g.linear_att ? a.lin_w[lane] : 0.f;
            attb = g.linear_att ? a.att_b[lane] : 0.f;
        }
        if (g.linear_att) {
            linb = a.lin_b[0];
            for (int e = lane; e < F * F; e += 64) aW[e] = a.att_W[e];
        }
    }
    if (wave == 0) {
        if (a.outer_conv && lane < CFFM_HEAD_UNITS) { d1b = a.d1_b[lane]; d2w = a.d2_w[lane]; }
        if (a.outer_conv) d2b = a.d2_b[0];
        if (tid == 0) {
            io = a.inner_conv ? a.inner_out[b] : 0.f;
            biasv = a.bias[0];
            yv = a.y ? a.y[b] : 0.f;
        }
    }
    if (a.outer_conv && !(POOLS && a.s0_ready)) {
        const float4* E4 = reinterpret_cast<const float4*>(a.Eo + (int64_t)b * F * D);
        for (int i = tid; i < F * D / 4; i += NTH) reinterpret_cast<float4*>(Et)[i] = E4[i];
    }
    float s0v = 0.f;                                                 // s0_ready: this thread's element of the pool, requested now
    if (POOLS && a.outer_conv && a.s0_ready && tid < D) s0v = a.t1[(int64_t)b * t1w + tid];
    if (wave == FO) {                                                // first-order term, :422-446 (needs nothing from the other waves)
        float lin;
        if (g.linear_att) {
            float z = attb;
            for (int gI = 0; gI < F; ++gI) {
                const float fg = __shfl(fbv, gI, 64);
                if (lane < F) z += fg * aW[gI * F + lane];          // staged by this wavefront above: no barrier needed
            }
            z = lane < F ? z / g.lamda_att : -INFINITY;
            const float mx = wave_max(z);
            const float e = lane < F ? expf(z - mx) : 0.f;
            const float den = wave_sum(e);
            const float at = e / den;
            if (lane < F) a.att[(int64_t)b * F + lane] = at;
            lin = wave_sum(lane < F ? fbv * at * linw : 0.f) + linb;
        } else {
            lin = wave_sum(fbv);
        }
        if (lane == 0) sc[1] = lin;
    }
    PHASE_MARK3(1);
    float o = 0.f;
    if (a.outer_conv) {
        // pools of the live layers: s_{l+1}[y] = sum_{x,q} act(C_l[b,y,x,q])                      (:390-391)
        int off = D;
        for (int l = 0; l < live; ++l) {                          // only s_1 .. s_{Lc-1} reach t1 (:394-396)
            const int S = D >> (l + 1);
            if (POOLS && !CL && a.pool_np[l] > 0) {                 // the conv epilogue left the partials: add them up in index order
                const int np = a.pool_np[l];
                for (int y = tid; y < S; y += NTH) {
                    const float* pp = a.pool[l] + ((int64_t)b * S + y) * np;
                    float v = 0.f;
                    for (int k = 0; k < np; ++k) v += pp[k];
                    t1s[off + y] = v;
                }
                off += S;
                continue;
            }
            const int n4 = S * Pp / 4;
            const float4* base = CL ? reinterpret_cast<const float4*>(smem + fused_c_off(l, c0_off, c1_off, D, Pp))
                                    : reinterpret_cast<const float4*>(a.C[l] + (int64_t)b * S * S * Pp);
            // wave w owns rows w, w+4, ...; four rows are swept together so that four loads are in flight per lane
            for (int y0 = wave; y0 < S; y0 += 16) {
                float s4[RPW];
#pragma unroll
                for (int u = 0; u < RPW; ++u) s4[u] = 0.f;
                for (int i = lane; i < n4; i += 64) {
#pragma unroll
                    for (int u = 0; u < RPW; ++u) {
                        const int yy = y0 + NW * u;
                        if (yy < S) {
                            const float4 v = base[(int64_t)yy * n4 + i];
                            s4[u] += (act_pos(v.x, act) + act_pos(v.y, act)) + (act_pos(v.z, act) + act_pos(v.w, act));
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < RPW; ++u) {
                    const float t = wave_sum(s4[u]);
                    if (lane == 0 && y0 + NW * u < S) t1s[off + y0 + NW * u] = t;
                }
            }
            off += S;
        }
        PHASE_MARK3(2);
        lds_barrier();                                             // Et (and the pools) are in LDS
        PHASE_MARK3(3);
        if (POOLS && a.s0_ready) {                                   // kernel-uniform: every thread takes the same side
            if (tid < D) t1s[tid] = s0v;                           // (D <= 256 <= NTH on this path: the tiled layer 0 has D <= 64)
        } else {
        for (int f = wave; f < F; f += NW) {                      // row sums of the embedding tile
            float s = 0.f;
            for (int d = lane; d < D; d += 64) s += Et[f * D + d];
            s = wave_sum(s);
            if (lane == 0) rs[f] = s;
        }
        lds_barrier();
        // s0[h] = sum_{w,p} Eo[i_p][h] * Eo[j_p][w] = sum_i Eo[i][h] * sum_{j>i} rowsum(j)   (:381)
        for (int h = tid; h < D; h += NTH) {
            float s = 0.f, R = 0.f;
            for (int i = F - 2; i >= 0; --i) {
                R += rs[i + 1];
                s = fmaf(Et[i * D + h], R, s);                       // spelled out: with F a constant the loop is unrolled and the
                                                                     // vectoriser pairs the products into v_pk_mul + add, unfused -
                                                                     // other bits than the run-time loop's fused multiply-adds
            }
            t1s[h] = s;
        }
        }
        lds_barrier();
        PHASE_MARK3(4);
        for (int k = tid; k < t1w; k += NTH) a.t1[(int64_t)b * t1w + k] = t1s[k];
        if (tid < 256) {                                             // dense(32), :409: 8 partial sums per unit
            float s = 0.f;
            if (pre) {
#pragma unroll
                for (int i = 0; i < HEAD_KPP; ++i) {
                    const int k = part * kpp + i;
                    if (i < kpp && k < t1w) s = fmaf(t1s[k], w1r[i], s);   // spelled out, as in the s0 pool below: the bound is a constant there
                }
            } else {
                for (int k = part * kpp; k < min(t1w, (part + 1) * kpp); ++k) s += t1s[k] * a.d1_w[k * CFFM_HEAD_UNITS + q];
            }
            hpart[part][q] = s;
        }
        lds_barrier();
        PHASE_MARK3(5);
        if (wave == 0) {                                             // + bias, then dense(1) * beta, :410, :414
            float h = 0.f;
            if (lane < CFFM_HEAD_UNITS) {
                h = d1b;
#pragma unroll
                for (int pp = 0; pp < 8; ++pp) h += hpart[pp][lane];
                a.h1[(int64_t)b * CFFM_HEAD_UNITS + lane] = h;
            }
            float v = lane < CFFM_HEAD_UNITS ? h * d2w : 0.f;
            v = wave_sum(v);
            if (lane == 0) sc[0] = g.beta_outer * (v + d2b);
        }
    }
    PHASE_MARK3(6);
    lds_barrier();
    if (tid == 0) {
        if (a.outer_conv) o = sc[0];
        float out = io;
        out += o;
        out += sc[1];
        out += biasv;                                                // :449-453
        float ev = out;
        if (a.y) a.sqerr[b] = loss_term(out, yv, a.loss, &ev);
        else if (a.loss == CFFM_LOSS_LOG) ev = 1.f / (1.f + expf(-out));
        a.out[b] = ev;
    }
}

struct HeadBwdArgs {
    Geo g;
    int B;
    int64_t Bg;
    const float *fb, *t1, *h1, *att, *out, *y, *Ctop;
    const float *d1_w, *d2_w, *att_W, *lin_w;
    float* scalars;
    const float* sqerr;      // non-NULL: sum the B local loss terms here instead of reading scalars[3]
    float* loss_out;         // may be NULL
    float *dout, *dt1, *dfb, *dCtop;
    float *s_attW, *s_attb, *s_bias, *s_d1w, *s_d1b, *s_d2w, *s_d2b, *s_linw, *s_linb;   // slab 0 pointers
    int64_t stride_front, stride_back;    // slab strides of the head-front (att_W, att_b, bias) and head-back ranges
    int64_t front_len, back_len;
    int loss, outer_conv;
    int unscaled;            // 1: leave the 1/L of the RMSE-style loss out of dout (data-parallel late scaling)
};

// The backward of the head is written as begin / loss / example / end so that the stand-alone kernel (one workgroup per
// slab looping over its examples) and the fused top-of-backward kernel share it.
struct HeadBwdState {
    float g_d2w, g_d1b, g_d2b, g_bias, g_linw, g_linb, g_attb;
    bool first;
};

__device__ __forceinline__ void head_bwd_begin(const HeadBwdArgs& a, int slab, HeadBwdState& st) {
    const int tid = threadIdx.x;
    float* s_attW = a.s_attW + (int64_t)slab * a.stride_front;
    float* s_d1w = a.s_d1w + (int64_t)slab * a.stride_back;
    // zero this slab's two ranges first (alignment gaps and members this configuration never writes)
    for (int64_t e = tid; e < a.front_len; e += 256) s_attW[e] = 0.f;        // att_W is the first member of the range
    for (int64_t e = tid; e < a.back_len; e += 256) s_d1w[e] = 0.f;          // d1_w is the first member of the range
    st.g_d2w = st.g_d1b = st.g_d2b = st.g_bias = st.g_linw = st.g_linb = st.g_attb = 0.f;
    st.first = true;
    __syncthreads();
}

// The loss L (CFFM.py:486-513) from the per-example terms, summed in the same fixed order by every workgroup; workgroup
// `publisher` also writes it out.  red: LDS [4].
__device__ __forceinline__ float head_bwd_loss(const HeadBwdArgs& a, bool publisher, float* red) {
    const int tid = threadIdx.x;
    float sum = 0.f, hybrid_log = 0.f;
    if (a.loss == CFFM_LOSS_HYBRID) {      // two sums with different normalisers: taken from out / y directly
        float p_sq = 0.f, p_log = 0.f;
        for (int i = tid; i < a.B; i += 256) {
            const float o = a.out[i], yy = a.y[i];
            p_sq += 0.5f * (yy - o) * (yy - o);
            p_log -= yy * logf(o + 1e-7f) + (1.f - yy) * logf(1.f - o + 1e-7f);
        }
        sum = block_sum<256>(p_sq, red);
        __syncthreads();
        hybrid_log = block_sum<256>(p_log, red);
        __syncthreads();
    } else if (a.unscaled) {
        sum = 0.f;           // not known yet: the caller all-reduces it together with the gradients
    } else if (a.sqerr) {    // same fixed-order sum in every workgroup
        float part = 0.f;
        for (int i = tid; i < a.B; i += 256) part += a.sqerr[i];
        sum = block_sum<256>(part, red);
        __syncthreads();
    } else {
        sum = a.scalars[3];
    }
    const float invB = 1.f / (float)a.Bg;
    float L;
    if (a.loss == CFFM_LOSS_SQUARE_RMSE) L = a.unscaled ? 1.f : sqrtf(sum * invB + 1e-10f);   // CFFM.py:493
    else if (a.loss == CFFM_LOSS_SQUARE_L2) L = sum;            // data term only (the regularisers are not summed here)
    else if (a.loss == CFFM_LOSS_HYBRID) L = 0.5f * sum + 0.5f * hybrid_log * invB;   // CFFM.py:511-513
    else L = sum * invB;
    if (publisher && tid == 0) {
        a.scalars[1] = L;
        if (a.sqerr) { a.scalars[0] = sum; a.scalars[3] = sum; }
        if (a.loss_out) a.loss_out[0] = L;
    }
    return L;
}

// dh1s [CFFM_HEAD_UNITS] and dt1s [2D-2] are LDS scratch of the caller
template <int ACTC = -1>
__device__ __forceinline__ void head_bwd_example(const HeadBwdArgs& a, int slab, HeadBwdState& st, int b, float d,
                                                 float* dh1s, float* dt1s) {
    const Geo& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t1w = 2 * g.D - 2;
    float* s_attW = a.s_attW + (int64_t)slab * a.stride_front;
    float* s_d1w = a.s_d1w + (int64_t)slab * a.stride_back;
    const bool first = st.first;
    int off_top = 0;
    for (int i = 0; i < g.live; ++i) off_top += g.D >> i;
    if (tid == 0) { a.dout[b] = d; st.g_bias += d; }
    __syncthreads();
    if (a.outer_conv) {
        const float dd = d * g.beta_outer;
        if (tid < CFFM_HEAD_UNITS) {
            const float v = dd * a.d2_w[tid];
            dh1s[tid] = v;
            st.g_d2w += a.h1[(int64_t)b * CFFM_HEAD_UNITS + tid] * dd;
            st.g_d1b += v;
        }
        if (tid == 0) st.g_d2b += dd;
        __syncthreads();
        for (int k = tid; k < t1w; k += 256) {
            float s = 0.f;
            for (int q = 0; q < CFFM_HEAD_UNITS; ++q) s += dh1s[q] * a.d1_w[k * CFFM_HEAD_UNITS + q];
            dt1s[k] = s;
            a.dt1[(int64_t)b * t1w + k] = s;
        }
        {   // dense(32) weight gradient, e = k * CFFM_HEAD_UNITS + q: a thread keeps its q while its k advances by 8 per trip; its t1
            // values are requested in batches of 8, ahead of the multiplies and stores
            static_assert(256 % CFFM_HEAD_UNITS == 0, "a thread's q does not change from trip to trip");
            const float* t1b = a.t1 + (int64_t)b * t1w;
            loads_first<8, 256, float>(tid, t1w * CFFM_HEAD_UNITS,
                [&](int e) { return t1b[e / CFFM_HEAD_UNITS]; },
                [&](int e, float t) {
                    const float v = t * dh1s[e % CFFM_HEAD_UNITS];
                    s_d1w[e] = first ? v : s_d1w[e] + v;
                });
        }
        __syncthreads();
        // gradient wrt the top live conv output: only its sum pool feeds the head
        const int ntop = 4 * g.Pp;
        for (int e = tid; e < ntop; e += 256) {
            const int yy = e / (2 * g.Pp);
            const int64_t idx = (int64_t)b * ntop + e;
            a.dCtop[idx] = dt1s[off_top + yy] * act_relu_grad(a.Ctop[idx], ACTC >= 0 ? ACTC : g.act);
        }
    }
    if (wave == 0) {
        const float fbv = lane < g.F ? a.fb[(int64_t)b * g.F + lane] : 0.f;
        if (g.linear_att) {
            const float at = lane < g.F ? a.att[(int64_t)b * g.F + lane] : 0.f;
            const float dg = lane < g.F ? d * a.lin_w[lane] : 0.f;
            const float da = dg * fbv;
            const float sda = wave_sum(da * at);
            const float dz = at * (da - sda) / g.lamda_att;
            float dfbv = dg * at;
            // The lane's row of att_W is requested first (12 at a time; F <= 11 under the fused top), then come the shuffles and the
            // sum with gI ascending, and the stores last: a store between two uses would make every use wait for it.
            constexpr int AW = 12;
            for (int g0 = 0; g0 < g.F; g0 += AW) {
                float aw[AW], dzg[AW];
#pragma unroll
                for (int u = 0; u < AW; ++u)
                    if (lane < g.F && g0 + u < g.F) aw[u] = a.att_W[lane * g.F + g0 + u];
#pragma unroll
                for (int u = 0; u < AW; ++u) dzg[u] = __shfl(dz, (g0 + u) & 63, 64);
                if (lane < g.F) {
#pragma unroll
                    for (int u = 0; u < AW; ++u)
                        if (g0 + u < g.F) dfbv += dzg[u] * aw[u];
#pragma unroll
                    for (int u = 0; u < AW; ++u) {
                        const int gI = g0 + u;
                        if (gI < g.F) {
                            const float v = fbv * dzg[u];
                            s_attW[lane * g.F + gI] = first ? v : s_attW[lane * g.F + gI] + v;
                        }
                    }
                }
            }
            if (lane < g.F) a.dfb[(int64_t)b * g.F + lane] = dfbv;
            st.g_linw += fbv * at * d;
            st.g_attb += dz;
            if (lane == 0) st.g_linb += d;
        } else if (lane < g.F) {
            a.dfb[(int64_t)b * g.F + lane] = d;
        }
    }
    st.first = false;
}

__device__ __forceinline__ void head_bwd_end(const HeadBwdArgs& a, int slab, const HeadBwdState& st) {
    const int tid = threadIdx.x;
    const int64_t sof = (int64_t)slab * a.stride_front, sob = (int64_t)slab * a.stride_back;
    if (tid < CFFM_HEAD_UNITS) {
        a.s_d2w[sob + tid] = st.g_d2w;
        a.s_d1b[sob + tid] = st.g_d1b;
    }
    if (tid < a.g.F) {
        a.s_linw[sob + tid] = st.g_linw;
        a.s_attb[sof + tid] = st.g_attb;
    }
    if (tid == 0) {
        a.s_d2b[sob] = st.g_d2b;
        a.s_bias[sof] = st.g_bias;
        a.s_linb[sob] = st.g_linb;
    }
}

// ---- single-example form (the fused top of the backward: one example per slab, 256 threads, Pp = 16 NT <= 64) -------------------
// Once d = dL/dout is known the head backward is three chains that share nothing but d.  In the looping form above wavefront 0
// carries all three one after the other, across three workgroup barriers; here each chain has wavefronts of its own, requests
// everything it reads in one batch and passes its intermediate values inside the wavefront, so there is no barrier in this function:
//   wavefront 0       (a) d -> dh -> dt1 -> dC_top, the only chain the input gradients wait for; keeps g_bias, g_d2w, g_d1b, g_d2b
//   wavefronts 1, 2   (b) the dense(32) weight-gradient slab, each thread with its own d * beta_outer * d2_w[q]
//   wavefront 3       (c) the attention / first-order branch; keeps g_linw, g_attb, g_linb
// Every sum keeps its operands and their order (q ascending in the transposed dense(32), gI ascending in the attention sum) and every
// slab element is stored as the looping form stores it for its first example: the results are the same bits.
// The caller's next workgroup barrier (__syncthreads) is what publishes dC_top to the other wavefronts.
template <int ACTC, int NT>
__device__ __forceinline__ void head_bwd_example_one(const HeadBwdArgs& a, int slab, HeadBwdState& st, int b, float d) {
    static_assert(NT >= 1 && NT <= 4, "dC_top is 4 Pp = 64 NT elements, NT per lane of wavefront 0; Pp <= 64 also means F <= 11");
    constexpr int HU = CFFM_HEAD_UNITS, CB = 128, UB = 16, AW = 12;    // threads of chain (b), its t1 values per thread and batch
    static_assert(CB % HU == 0, "a thread's q does not change from element to element");
    const Geo& g = a.g;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t1w = 2 * g.D - 2;
    if (wave == 0) {
        if (lane == 0) { a.dout[b] = d; st.g_bias += d; }
        if (a.outer_conv) {
            const float dd = d * g.beta_outer;
            int off_top = 0;
            for (int i = 0; i < g.live; ++i) off_top += g.D >> i;
            const float* Ct = a.Ctop + (int64_t)b * (64 * NT);
            // requests of the whole chain (lanes past an array's end read its last element again and drop it)
            const float d2wv = a.d2_w[lane & (HU - 1)];
            const float h1v = a.h1[(int64_t)b * HU + (lane & (HU - 1))];
            float ct[NT];
#pragma unroll
            for (int u = 0; u < NT; ++u) ct[u] = Ct[lane + 64 * u];
            float w[HU];                                             // this lane's row k = lane of the dense(32) kernel
            {
                const float* r = a.d1_w + min(lane, t1w - 1) * HU;
#pragma unroll
                for (int q = 0; q < HU; ++q) w[q] = r[q];
            }
            const float dhv = dd * d2wv;                               // dh[q] on lane q (and once more on lane q + 32)
            st.g_d2w += h1v * dd;                                      // on every lane (head_bwd_end_one stores lanes 0 .. 31): under a
            st.g_d1b += dhv;                                           // lane condition hipcc sinks the h1 load behind the wait for d2_w
            if (lane == 0) st.g_d2b += dd;
            float dtop[2] = {0.f, 0.f};                                // dt1[off_top], dt1[off_top + 1]: all of dt1 that dC_top needs
            // One trip up to D = 32.  At D = 64 a lane carries a second k = lane + 64, whose row is fetched when its trip comes: holding
            // both rows at once costs the Pp = 16 instances a wavefront per SIMD (81 registers against 79).
            // (do-while: t1w >= 14, and behind a loop guard hipcc sinks the row's loads under the guard, behind the wait for d2_w)
            int k0 = 0;
            do {
                if (k0 > 0) {
                    const float* r = a.d1_w + min(k0 + lane, t1w - 1) * HU;
#pragma unroll
                    for (int q = 0; q < HU; ++q) w[q] = r[q];
                }
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < HU; ++q)                           // q is uniform: dh[q] comes out of lane q by v_readlane
                    s = fmaf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dhv), q)), w[q], s);   // spelled
                                                                       // out: the fused multiply-add the looping form's loop compiles to
                if (k0 + lane < t1w) a.dt1[(int64_t)b * t1w + k0 + lane] = s;
#pragma unroll
                for (int yy = 0; yy < 2; ++yy) {
                    const int kk = off_top + yy - k0;                  // uniform
                    if (kk >= 0 && kk < 64) dtop[yy] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), kk));
                }
                k0 += 64;
            } while (k0 < t1w);
            // gradient wrt the top live conv output: only its sum pool feeds the head
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const int e = lane + 64 * u, yy = e / (32 * NT);       // e / (2 Pp)
                a.dCtop[(int64_t)b * (64 * NT) + e] = (yy ? dtop[1] : dtop[0]) * act_relu_grad(ct[u], ACTC >= 0 ? ACTC : g.act);
            }
        }
    } else if (wave == 3) {
        float* s_attW = a.s_attW + (int64_t)slab * a.stride_front;
        // requests without a lane condition (lanes and columns past F read the last one again and drop it): one basic block, so that
        // nothing waits between them
        const int fl = min(lane, g.F - 1);
        const float fbr = a.fb[(int64_t)b * g.F + fl];
        const float fbv = lane < g.F ? fbr : 0.f;
        if (g.linear_att) {
            const float atr = a.att[(int64_t)b * g.F + fl], lwr = a.lin_w[fl];
            float aw[AW], dzg[AW];                                     // the lane's row of att_W (F <= 11 < AW), requested with the rest
#pragma unroll
            for (int u = 0; u < AW; ++u) aw[u] = a.att_W[fl * g.F + min(u, g.F - 1)];
            const float at = lane < g.F ? atr : 0.f;
            const float lw = lane < g.F ? lwr : 0.f;
            const float dg = lane < g.F ? d * lw : 0.f;
            const float da = dg * fbv;
            const float sda = wave_sum(da * at);
            const float dz = at * (da - sda) / g.lamda_att;
            float dfbv = dg * at;
#pragma unroll
            for (int u = 0; u < AW; ++u) dzg[u] = __shfl(dz, u, 64);
#pragma unroll
            for (int u = 0; u < AW; ++u) pin(aw[u]);                   // their only use is under the lane condition below
            if (lane < g.F) {
#pragma unroll
                for (int u = 0; u < AW; ++u)
                    if (u < g.F) dfbv = fmaf(dzg[u], aw[u], dfbv);    // spelled out: left to hipcc, the first term here became
                                                                       // fma(dg, at, dzg[0] * aw[0]), one rounding elsewhere
#pragma unroll
                for (int u = 0; u < AW; ++u)
                    if (u < g.F) s_attW[lane * g.F + u] = fbv * dzg[u];
                a.dfb[(int64_t)b * g.F + lane] = dfbv;
            }
            st.g_linw += fbv * at * d;
            st.g_attb += dz;
            if (lane == 0) st.g_linb += d;
        } else if (lane < g.F) {
            a.dfb[(int64_t)b * g.F + lane] = d;
        }
    } else if (a.outer_conv) {
        // dense(32) weight gradient, e = k * CFFM_HEAD_UNITS + q, over the 128 threads of wavefronts 1 and 2: a thread keeps its q while
        // its k advances by 4 per element; its first UB values of t1 are requested with its d2_w[q], any further ones (D >= 64) in batches
        float* s_d1w = a.s_d1w + (int64_t)slab * a.stride_back;
        const float* t1b = a.t1 + (int64_t)b * t1w;
        const int t = (int)threadIdx.x - 64, n = t1w * HU;
        const float d2wv = a.d2_w[t & (HU - 1)];
        float tv[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) tv[u] = t1b[min(t + CB * u, n - 1) / HU];
        const float dd = d * g.beta_outer;
        const float v = dd * d2wv;                                     // the same two multiplies as dh[q] of chain (a): the same bits
        // every product first, pinned: a product formed under its store's condition takes its wait there, where the stores issued so
        // far count as outstanding too, so that the later stores wait for the earlier ones to be acknowledged
#pragma unroll
        for (int u = 0; u < UB; ++u) { tv[u] *= v; pin(tv[u]); }
#pragma unroll
        for (int u = 0; u < UB; ++u)
            if (t + CB * u < n) s_d1w[t + CB * u] = tv[u];
        if (n > UB * CB)
            loads_first<UB, CB, float>(t, n - UB * CB,
                [&](int e) { return t1b[(e + UB * CB) / HU]; },
                [&](int e, float tt) { s_d1w[e + UB * CB] = tt * v; });
    }
}

// the slab's per-example sums, stored from the lanes head_bwd_example_one keeps them on
__device__ __forceinline__ void head_bwd_end_one(const HeadBwdArgs& a, int slab, const HeadBwdState& st) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t sof = (int64_t)slab * a.stride_front, sob = (int64_t)slab * a.stride_back;
    if (wave == 0) {
        if (lane < CFFM_HEAD_UNITS) {
            a.s_d2w[sob + lane] = st.g_d2w;
            a.s_d1b[sob + lane] = st.g_d1b;
        }
        if (lane == 0) {
            a.s_d2b[sob] = st.g_d2b;
            a.s_bias[sof] = st.g_bias;
        }
    } else if (wave == 3) {
        if (lane < a.g.F) {
            a.s_linw[sob + lane] = st.g_linw;
            a.s_attb[sof + lane] = st.g_attb;
        }
        if (lane == 0) a.s_linb[sob] = st.g_linb;
    }
}

// Head of the CFFM graph: sum pooling over the conv stack (CFFM.py:381, :390-396), the two dense
// layers of the outer branch (:409-414), the linear-attention first-order term (:422-446), add_n (:453),
// the loss terms (:486-514) and all of their gradients.
//
// Everything here is tiny per example except the pooling sweep, which re-reads the conv outputs once
// (contiguous S*Pp-float rows, 16-byte loads) - HBM/L2-bound and bitwise reproducible (fixed tree).
#include "internal.hpp"

#include "head_body.hpp"

__global__ __launch_bounds__(256) void head_fwd_kernel(HeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    head_fwd_body<4, -1, true>(a, blockIdx.x, smem);
}

// deterministic single-workgroup sum of n floats -> dst[0] (and dst[3] when mirror != 0)
__global__ __launch_bounds__(1024) void sum_kernel(const float* __restrict__ x, int64_t n, float* dst, int mirror) {
    __shared__ float red[16];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += x[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        dst[0] = s;
        if (mirror) dst[3] = s;
    }
}

__global__ __launch_bounds__(256) void head_bwd_kernel(HeadBwdArgs a) {
    __shared__ float dh1s[CFFM_HEAD_UNITS];
    __shared__ float dt1s[1024];
    __shared__ float red[4];
    HeadBwdState st;
    head_bwd_begin(a, blockIdx.x, st);
    const float L = head_bwd_loss(a, blockIdx.x == 0, red);
    const float invB = 1.f / (float)a.Bg;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x)
        head_bwd_example(a, blockIdx.x, st, b, head_dout(a.loss, a.out[b], a.y[b], invB, L), dh1s, dt1s);
    head_bwd_end(a, blockIdx.x, st);
}

// The same backward from a dL/dout the caller hands in (cffm_backward_dout): no loss is formed, so neither scalars[3], sqerr, out nor y
// is read, and nothing is normalised - every gradient is linear in dout[b].
__global__ __launch_bounds__(256) void head_bwd_dout_kernel(HeadBwdArgs a, const float* __restrict__ dout_in) {
    __shared__ float dh1s[CFFM_HEAD_UNITS];
    __shared__ float dt1s[1024];
    HeadBwdState st;
    head_bwd_begin(a, blockIdx.x, st);
    for (int b = blockIdx.x; b < a.B; b += gridDim.x)
        head_bwd_example(a, blockIdx.x, st, b, dout_in[b], dh1s, dt1s);
    head_bwd_end(a, blockIdx.x, st);
}

HeadArgs StepCtx::head_args(const float* y, bool s0_ready) const {
    HeadArgs a{};
    a.g = g; a.B = B;
    a.Eo = at<const float>(wl.Eo); a.fb = at<const float>(wl.fb); a.inner_out = at<const float>(wl.inner_out);
    for (int l = 0; l < CFFM_MAX_LAYERS; ++l) a.C[l] = at<const float>(wl.C[l]);
    a.d1_w = theta + tl.d1_w; a.d1_b = theta + tl.d1_b; a.d2_w = theta + tl.d2_w; a.d2_b = theta + tl.d2_b;
    a.att_W = theta + tl.att_W; a.att_b = theta + tl.att_b; a.lin_w = theta + tl.lin_w; a.lin_b = theta + tl.lin_b;
    a.bias = theta + tl.bias;
    a.y = y;
    a.t1 = at(wl.t1); a.h1 = at(wl.h1); a.att = at(wl.att); a.out = at(wl.out); a.sqerr = at(wl.sqerr);
    a.loss = s->loss; a.inner_conv = s->inner_conv; a.outer_conv = s->outer_conv;
    a.s0_ready = (s0_ready && s->outer_conv && s->D <= 256) ? 1 : 0;
    for (int l = 0; l < CFFM_MAX_LAYERS; ++l) {       // wide shapes only (pool_partials); the fused forward reads neither
        a.pool_np[l] = wl.pool_np[l];
        a.pool[l] = wl.pool_np[l] > 0 ? at<const float>(wl.pool[l]) : nullptr;
    }
    return a;
}

HeadBwdArgs StepCtx::head_bwd_args(const float* y, int64_t B_global, const BwdOpts& o) const {
    const SlabRange& rf = sp.r[sp.head_front];
    const SlabRange& rb = sp.r[sp.head_back];
    float* gf = at(wl.gpart) + rf.base - rf.off;        // slab 0 of theta offset x lives at gf + x
    float* gb = at(wl.gpart) + rb.base - rb.off;
    HeadBwdArgs a{};
    a.g = g; a.B = B; a.Bg = B_global;
    a.fb = at<const float>(wl.fb); a.t1 = at<const float>(wl.t1); a.h1 = at<const float>(wl.h1);
    a.att = at<const float>(wl.att); a.out = at<const float>(wl.out); a.y = y;
    const int top = g.live - 1;
    a.Ctop = at<const float>(wl.C[top]); a.dCtop = at(wl.dC[top]);
    a.d1_w = theta + tl.d1_w; a.d2_w = theta + tl.d2_w; a.att_W = theta + tl.att_W; a.lin_w = theta + tl.lin_w;
    a.scalars = at(wl.scalars);
    a.sqerr = o.local_sum() ? at<const float>(wl.sqerr) : nullptr;
    a.loss_out = o.loss_out;
    a.dout = at(wl.dout); a.dt1 = at(wl.dt1); a.dfb = at(wl.dfb);
    a.s_attW = gf + tl.att_W; a.s_attb = gf + tl.att_b; a.s_bias = gf + tl.bias;
    a.s_d1w = gb + tl.d1_w; a.s_d1b = gb + tl.d1_b; a.s_d2w = gb + tl.d2_w; a.s_d2b = gb + tl.d2_b;
    a.s_linw = gb + tl.lin_w; a.s_linb = gb + tl.lin_b;
    a.stride_front = rf.len; a.stride_back = rb.len; a.front_len = rf.len; a.back_len = rb.len;
    a.loss = s->loss; a.outer_conv = s->outer_conv; a.unscaled = o.unscaled ? 1 : 0;
    return a;
}

extern "C" int cffm_head_fwd(const cffm_shape_t* s, const float* theta, void* ws, const float* y, int32_t B, void* stream) {
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    return cffm_head_fwd_impl(StepCtx(s, B, theta, ws), y, HeadFwdOpts(), (hipStream_t)stream);
}

int cffm_head_fwd_impl(const StepCtx& c, const float* y, const HeadFwdOpts& o, hipStream_t stream) {
    if (2 * c.g.D - 2 > 1024) return CFFM_ERR_UNSUPPORTED;
    int rc = check_lds(c.s);
    if (rc) return rc;
    const size_t lds = head_fwd_lds(c.g);          // above 64 KB from F * D + F * F > 15,032 on (F >= 50 at D = 256, F >= 28 at D = 512)
    if ((rc = set_lds(head_fwd_kernel, lds))) return rc;
    const HeadArgs a = c.head_args(y, o.s0_ready);
    hipLaunchKernelGGL(head_fwd_kernel, dim3(c.B), dim3(256), lds, stream, a);
    CFFM_CHECK_LAUNCH();
    if (y && o.sum_loss) {
        hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(1024), 0, stream, c.at<const float>(c.wl.sqerr), (int64_t)c.B,
                           c.at(c.wl.scalars), 1);
        CFFM_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int cffm_head_bwd(const cffm_shape_t* s, const float* theta, void* ws, const float* y, int32_t B,
                             int64_t B_global, void* stream) {
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    return cffm_head_bwd_impl(StepCtx(s, B, theta, ws), y, B_global, BwdOpts(), (hipStream_t)stream);
}

int cffm_head_bwd_impl(const StepCtx& c, const float* y, int64_t B_global, const BwdOpts& o, hipStream_t stream) {
    if (2 * c.g.D - 2 > 1024) return CFFM_ERR_UNSUPPORTED;
    int rc = check_lds(c.s);
    if (rc) return rc;
    const HeadBwdArgs a = c.head_bwd_args(y, B_global, o);
    if (o.dout_in) hipLaunchKernelGGL(head_bwd_dout_kernel, dim3(small_slabs(c.B)), dim3(256), 0, stream, a, o.dout_in);
    else hipLaunchKernelGGL(head_bwd_kernel, dim3(small_slabs(c.B)), dim3(256), 0, stream, a);
    CFFM_CHECK_LAUNCH();
    return 0;
}

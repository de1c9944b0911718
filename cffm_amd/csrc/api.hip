// Layout queries and the composite entry points (what CFFM.evaluate / CFFM.train call in place of the
// two sess.run()s, CFFM.py:200 and :596).
#include "internal.hpp"

#include <string.h>

extern "C" int cffm_abi_version(void) { return CFFM_ABI_VERSION; }

extern "C" const char* cffm_error_string(int err) {
    switch (err) {
        case 0: return "ok";
        case CFFM_ERR_BAD_SHAPE: return "cffm: bad shape / argument";
        case CFFM_ERR_UNSUPPORTED: return "cffm: unsupported configuration";
        default: return hipGetErrorString((hipError_t)err);
    }
}

extern "C" int cffm_theta_layout(const cffm_shape_t* s, cffm_theta_layout_t* out) {
    int rc = check_shape(s);
    if (rc) return rc;
    memset(out, 0, sizeof(*out));
    const Geo g = make_geo(s);
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += (n + 3) / 4 * 4; return r; };   // 16-byte aligned members
    out->att_W = take((int64_t)g.F * g.F);
    out->att_b = take(g.F);
    out->bias = take(1);
    out->inner_cw = take(4);
    out->inner_cb = take(2);
    out->inner_dw = take((int64_t)g.P * g.K);
    out->inner_db = take(1);
    for (int l = 0; l < g.live; ++l) {
        out->conv_w[l] = take((int64_t)4 * g.Pp * g.Pp);     // [tap][Pp][Pp], zero outside [P][P]
        out->conv_b[l] = take(g.Pp);
    }
    out->d1_w = take((int64_t)(2 * g.D - 2) * CFFM_HEAD_UNITS);
    out->d1_b = take(CFFM_HEAD_UNITS);
    out->d2_w = take(CFFM_HEAD_UNITS);
    out->d2_b = take(1);
    out->lin_w = take(g.F);
    out->lin_b = take(1);
    out->n = o;
    out->P = g.P; out->Pp = g.Pp; out->Lc = g.Lc; out->live = g.live;
    return 0;
}

extern "C" int cffm_ws_layout(const cffm_shape_t* s, int32_t B, cffm_ws_layout_t* out) {
    int rc = check_shape(s);
    if (rc) return rc;
    if (B < 1) return CFFM_ERR_BAD_SHAPE;
    cffm_theta_layout_t tl;
    cffm_theta_layout(s, &tl);
    SlabPlan sp;
    make_slab_plan(s, B, tl, &sp);
    return cffm_ws_layout_from(s, B, tl, sp, out);
}

// the workspace layout for a theta layout and slab plan the caller already has (StepCtx); shape checked, B >= 1
int cffm_ws_layout_from(const cffm_shape_t* s, int32_t B, const cffm_theta_layout_t& tl, const SlabPlan& sp, cffm_ws_layout_t* out) {
    memset(out, 0, sizeof(*out));
    const Geo g = make_geo(s);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { int64_t r = o; o += (bytes + 255) / 256 * 256; return r; };
    const int64_t b = B;
    out->gpart = take(sp.total * 4);                             // first: offset 0
    out->gpart_floats = sp.total;
    out->scalars = take(16 * 4);
    out->Ei = take(b * g.F * g.K * 4);
    out->Eo = take(b * g.F * g.D * 4);
    out->fb = take(b * g.F * 4);
    out->inner_out = take(b * 4);
    for (int l = 0; l < g.live; ++l) {
        const int64_t S = g.D >> (l + 1);
        out->C[l] = take(b * S * S * g.Pp * 4);
    }
    out->t1 = take(b * (2 * g.D - 2) * 4);
    out->h1 = take(b * CFFM_HEAD_UNITS * 4);
    out->att = take(b * g.F * 4);
    out->out = take(b * 4);
    out->sqerr = take(b * 4);
    out->dout = take(b * 4);
    out->dt1 = take(b * (2 * g.D - 2) * 4);
    for (int l = 0; l < g.live; ++l) {
        const int64_t S = g.D >> (l + 1);
        out->dC[l] = take(b * S * S * g.Pp * 4);
    }
    out->dEi = take(b * g.F * g.K * 4);
    out->dEo = take(b * g.F * g.D * 4);
    out->dfb = take(b * g.F * 4);
    const int64_t nrows = b * g.F;
    out->sort_keys = take(nrows * 8);                            // packed (id << 32 | slot), unsorted
    out->sort_vals = take(nrows * 8);                            // the same keys, sorted
    out->sort_tmp_bytes = nrows * 32 + (4 << 20);
    out->sort_tmp = take(out->sort_tmp_bytes);
    if (s->loss == CFFM_LOSS_SQUARE_L2 || s->optimizer == CFFM_OPT_ADAM) {   // dense table gradients
        out->Gi = take((int64_t)s->M * s->K * 4);
        out->Go = take((int64_t)s->M * s->D * 4);
        out->Gfb = take((int64_t)s->M * 4);
    }
    if (s->outer_conv) {
        for (int l = 0; l < g.live; ++l) {
            const int np = pool_partials(g, l);
            out->pool_np[l] = np;
            if (np > 0) out->pool[l] = take(b * (g.D >> (l + 1)) * np * 4);
        }
        if (conv0_tile_dgrad2_ok(g)) {                           // WA + WE of conv0_fact_tile_dgrad2_kernel (conv.hip)
            out->w0pack_floats = 2 * (int64_t)(2 * g.F) * (g.Pp / 16) * 1024;
            out->w0pack = take(out->w0pack_floats * 4);
            if (g.live > 1 && g.act != CFFM_ACT_GELU)        // relu mask of C[0] (gelu's derivative needs the value)
                out->relu0 = take(relu_mask_off(g, b, g.live - 1));       // masks of C_0 .. C_{live-2}
        }
        if (g.Pp > 64 && g.live > 1) {                           // the bf16x3 loops of the direct layers: one pre-split filter image
            out->wb3_bytes = cffm_wb3_bytes(g.Pp);
            out->wb3 = take(out->wb3_bytes);
        }
    }
    out->bytes = o;
    return 0;
}

// One context per ABI call: every entry point below checks the shape, returns early for an empty batch and then builds the
// StepCtx (layouts, slab plan) that forward_impl / backward_impl and every launcher under them share.
//
// no_materialise: the composites that own the whole step (cffm_train_step, cffm_predict, cffm_dp_local) let the wide shapes
// consume the looked-up rows in the kernel that fetches them (cffm_gather_inner_fwd_wide) and re-fetch them from the tables
// where a later kernel needs them (backward_impl with BwdOpts.rows = the same tab / ids); ws.Ei / ws.Eo are then never written.
// cffm_forward keeps materialising: its callers (the stage-by-stage parity tests, cffm_backward, the row-sharded step) read
// ws.Ei / ws.Eo afterwards.
static bool wide_rows(const cffm_shape_t* s, const RowTables& r) { return r.tab && r.ids && cffm_wide_regather_ok(s); }
// the rows of one table as the wide kernels fetch them: straight from the table, or (stride / records > 0) out of packed records
static RowSrc table_rows(const cffm_shape_t* s, const float* base, const RowTables& r) {
    return {base, r.ids, r.records > 0 ? r.records : s->M, r.stride};
}
static RowTables step_rows(const cffm_tables_t* tab, const int32_t* ids, int stride = 0, int records = 0) {
    RowTables r;
    r.tab = tab; r.ids = ids; r.stride = stride; r.records = records;
    return r;
}

struct FwdOpts {
    bool fused_step = false;         // part of a train step: no separate loss sum, the gather also emits the sort keys
    bool no_materialise = false;     // see above
};
// rows.tab == NULL: row-sharded tables, the rows are already staged in ws.Ei / ws.Eo / ws.fb
static int forward_impl(const StepCtx& c, const RowTables& rows, const float* y, hipStream_t stream, const FwdOpts& o = FwdOpts()) {
    const cffm_shape_t* s = c.s;
    const cffm_tables_t* tab = rows.tab;
    const cffm_ws_layout_t& wl = c.wl;
    HeadFwdOpts ho;
    ho.sum_loss = !o.fused_step;
    int rc = cffm_route_check(c);        // a kernel of this shape's step cannot fit a CU's LDS: refused before the first launch
    if (rc) return rc;
    if (o.no_materialise && wide_rows(s, rows)) {
        if ((rc = cffm_gather_inner_fwd_wide(c, rows, stream))) return rc;
        const RowSrc ro = table_rows(s, tab->outer_emb, rows);
        if ((rc = cffm_conv_fwd_impl(c, 0, stream, &ro))) return rc;
        for (int l = 1; l < c.g.live; ++l)
            if ((rc = cffm_conv_fwd_impl(c, l, stream))) return rc;
        ho.s0_ready = true;
        return cffm_head_fwd_impl(c, y, ho, stream);
    }
    if (!tab) {
        if (o.fused_step) return CFFM_ERR_UNSUPPORTED;
        if ((rc = cffm_inner_fwd_impl(c, nullptr, nullptr, stream))) return rc;
    } else if (o.fused_step && s->inner_conv && s->outer_conv) {
        // the inner-branch kernel gathers the rows of its example itself (one launch less)
        if ((rc = cffm_inner_fwd_impl(c, tab, rows.ids, stream))) return rc;
    } else {
        rc = cffm_gather_impl(s, tab, rows.ids, c.B, s->inner_conv ? c.at(wl.Ei) : nullptr, s->outer_conv ? c.at(wl.Eo) : nullptr,
                              c.at(wl.fb), o.fused_step ? c.at<unsigned long long>(wl.sort_keys) : nullptr, stream);
        if (rc) return rc;
        if ((rc = cffm_inner_fwd_impl(c, nullptr, nullptr, stream))) return rc;
    }
    for (int l = 0; l < c.g.live && s->outer_conv; ++l)
        if ((rc = cffm_conv_fwd_impl(c, l, stream))) return rc;
    return cffm_head_fwd_impl(c, y, ho, stream);
}

extern "C" int cffm_forward(const cffm_shape_t* s, const cffm_tables_t* tab, const float* theta, const int32_t* ids,
                            const float* y, int32_t B, void* ws, void* stream) {
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    const StepCtx c(s, B, theta, ws);
    return forward_impl(c, step_rows(tab, ids), y, (hipStream_t)stream);
}

extern "C" int cffm_predict(const cffm_shape_t* s, const cffm_tables_t* tab, const float* theta, const int32_t* ids,
                            int32_t B, void* ws, float* out, void* stream) {
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    const StepCtx c(s, B, theta, ws);
    FwdOpts fo;
    fo.no_materialise = true;
    // Where the train step runs its forward in one launch (cffm_fwd_all_ok), predict runs that launch too, without labels and without
    // the key placement: one launch instead of one per stage, and `out` is the train step's `out` on the same ids bit for bit.
    if (tab && ids && cffm_fwd_all_ok(s, B)) rc = cffm_fwd_all_impl(c, tab, ids, nullptr, (hipStream_t)stream, false);
    else rc = forward_impl(c, step_rows(tab, ids), nullptr, (hipStream_t)stream, fo);
    if (rc || !out) return rc;
    hipError_t e = hipMemcpyAsync(out, c.at(c.wl.out), (size_t)B * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return e == hipSuccess ? 0 : (int)e;
}

// backward through the slab reduction (BwdOpts, internal.hpp)
static int backward_impl(const StepCtx& c, const float* y, int64_t B_global, float* grad, hipStream_t stream,
                         const BwdOpts& o = BwdOpts()) {
    const cffm_shape_t* s = c.s;
    const int32_t B = c.B;
    int rc = cffm_route_check(c);        // as in forward_impl (also covers the inner-branch roles of bwd_top / conv_bwd_pair)
    if (rc) return rc;
    if (o.dout_fused && (o.dout_in || !bwd_top_ok(s, B) || s->loss == CFFM_LOSS_SQUARE_L2)) return CFFM_ERR_UNSUPPORTED;   // no fused top there
    if (!s->inner_conv || !s->outer_conv || !s->linear_att) {   // slabs of a disabled branch must read as zeros
        hipError_t e = hipMemsetAsync(c.at(c.wl.gpart), 0, (size_t)c.wl.gpart_floats * 4, stream);
        if (e != hipSuccess) return (int)e;
    }
    bool inner_done = false;
    const bool wide = wide_rows(s, o.rows);          // the forward did not materialise Ei / Eo: rows come from the tables (RowSrc)
    // a caller's dL/dout (o.dout_in) always takes the stage route below: bwd_top / conv01_bwd form dL/dout from (out, y, L) themselves.
    // o.dout_fused is the caller's dL/dout on the fused route (the DOUT instances of bwd_top; nothing below it looks at the loss)
    if (!o.dout_in && bwd_top_ok(s, B) && s->loss != CFFM_LOSS_SQUARE_L2) {
        // head + top two conv layers + inner branch: one launch
        int next = 0;
        if ((rc = cffm_bwd_top_impl(c, y, B_global, o, stream, &next))) return rc;
        inner_done = true;
        if (bwd_fused01_ok(s, B)) {            // layers 3..0 below the fused top: one launch
            if ((rc = cffm_conv01_bwd_impl(c, stream))) return rc;
            next = -1;
        }
        for (int l = next; l >= 0; --l) {
            ConvBwdOpts co;
            co.with_top_wgrad = l == next && top_wgrad_deferred(s, B);     // (never layer 0: conv_pair_ok wants l >= 1)
            if ((rc = cffm_conv_bwd_impl(c, l, stream, co))) return rc;
        }
    } else {
        if ((rc = cffm_head_bwd_impl(c, y, B_global, o, stream))) return rc;
        const RowSrc ro = table_rows(s, wide ? o.rows.tab->outer_emb : nullptr, o.rows);
        for (int l = c.g.live - 1; l >= 0 && s->outer_conv; --l) {
            ConvBwdOpts co;
            if (l == c.g.live - 1) co.carry_inner = &inner_done;    // a paired launch (layers >= 1 only) takes the inner branch along
            if (l == 0 && wide) co.rs = &ro;
            if ((rc = cffm_conv_bwd_impl(c, l, stream, co))) return rc;
        }
    }
    if (!inner_done) {
        const RowSrc ri = table_rows(s, wide ? o.rows.tab->inner_emb : nullptr, o.rows);
        if ((rc = cffm_inner_bwd_rows(c, wide ? &ri : nullptr, stream))) return rc;
    }
    if (o.skip_reduce) return 0;
    return cffm_reduce_slabs_impl(c, grad, o.adagrad_theta, o.adagrad_acc, s->lr, stream);
}

extern "C" int cffm_backward(const cffm_shape_t* s, const float* theta, const float* y, int32_t B, int64_t B_global,
                             void* ws, float* grad, void* stream) {
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    const StepCtx c(s, B, theta, ws);
    return backward_impl(c, y, B_global, grad, (hipStream_t)stream);
}

// Backward from the caller's dL/dout (include/cffm_hip.h): what a loss that couples the examples of a batch, or one written outside
// the library, needs.  The forward was cffm_forward (rows materialised); s->loss is accepted and not used.
extern "C" int cffm_backward_dout(const cffm_shape_t* s, const float* theta, const float* dout, int32_t B, void* ws, float* grad,
                                  void* stream) {
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    if (!theta || !dout || !ws || !grad) return CFFM_ERR_BAD_SHAPE;
    const StepCtx c(s, B, theta, ws);
    BwdOpts bo;
    bo.dout_in = dout;
    return backward_impl(c, nullptr, (int64_t)B, grad, (hipStream_t)stream, bo);
}

// The same from the caller's dL/dout on the launches cffm_backward takes where the fused top runs (include/cffm_hip.h): bwd_top as its
// DOUT instance, then conv01_bwd or the pair / stage launches below it, then the slab reduction.
extern "C" int cffm_backward_dout_fused(const cffm_shape_t* s, const float* theta, const float* dout, int32_t B, void* ws, float* grad,
                                        void* stream) {
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    if (!theta || !dout || !ws || !grad) return CFFM_ERR_BAD_SHAPE;
    const StepCtx c(s, B, theta, ws);
    BwdOpts bo;
    bo.dout_fused = dout;
    return backward_impl(c, nullptr, (int64_t)B, grad, (hipStream_t)stream, bo);
}

// this rank's loss-term sum (ws.scalars[0]) -> grad[theta.n], so that ONE all-reduce carries gradients and loss
static int move_loss_sum(const StepCtx& c, float* grad, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(grad + c.tl.n, c.at(c.wl.scalars), sizeof(float), hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? 0 : (int)e;
}

// Data-parallel backward: dL/dout = (out - y) / B_global WITHOUT the 1/L of the RMSE-style loss; grad must have room
// for theta.n + 4 floats - element theta.n receives this rank's loss-term sum so that ONE all-reduce carries both.
// cffm_dp_apply then applies 1/L to the summed gradients.  The packed rows for the all-gather are written to `rows`
// [B*F][1 + K + D + 1] = (id bits | dEi | dEo | dfb).
extern "C" int cffm_backward_unscaled(const cffm_shape_t* s, const float* theta, const int32_t* ids, const float* y,
                                      int32_t B, int64_t B_global, void* ws, float* grad, float* rows, void* stream) {
    if (s && (s->loss == CFFM_LOSS_HYBRID || s->loss == CFFM_LOSS_SQUARE_L2)) return CFFM_ERR_UNSUPPORTED;   // single-process only
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    const StepCtx c(s, B, theta, ws);
    BwdOpts bo;
    bo.unscaled = true;
    if ((rc = backward_impl(c, y, B_global, grad, (hipStream_t)stream, bo))) return rc;
    if (!rows) return move_loss_sum(c, grad, (hipStream_t)stream);   // the caller packs the row gradients itself (cffm_pack_rows_dedup)
    return cffm_pack_rows(c, ids, grad + c.tl.n, rows, (hipStream_t)stream);
}

// ---- row-sharded step without staging (cffm_amd/dist.py ShardedStep): the packed records a rank received ARE the tables ------
static bool packed_view(const cffm_shape_t* s, const float* packed, int64_t n_records, cffm_tables_t* view) {
    if (check_shape(s) || !packed || n_records <= 0 || n_records >= (1ll << 31) || !cffm_wide_regather_ok(s)) return false;
    view->inner_emb = const_cast<float*>(packed);
    view->outer_emb = const_cast<float*>(packed) + s->K;
    view->feat_bias = const_cast<float*>(packed) + s->K + s->D;
    return true;
}
extern "C" int cffm_forward_packed(const cffm_shape_t* s, const float* theta, const float* packed, const int32_t* pos,
                                   int64_t n_records, const float* y, int32_t B, void* ws, void* stream) {
    cffm_tables_t view;
    if (B <= 0) return check_shape(s);
    if (!pos || !packed_view(s, packed, n_records, &view)) return CFFM_ERR_UNSUPPORTED;
    const StepCtx c(s, B, theta, ws);
    FwdOpts fo;
    fo.no_materialise = true;
    return forward_impl(c, step_rows(&view, pos, s->K + s->D + 4, (int)n_records), y, (hipStream_t)stream, fo);
}
extern "C" int cffm_backward_unscaled_packed(const cffm_shape_t* s, const float* theta, const float* packed, const int32_t* pos,
                                             int64_t n_records, const float* y, int32_t B, int64_t B_global, void* ws, float* grad,
                                             void* stream) {
    if (s && (s->loss == CFFM_LOSS_HYBRID || s->loss == CFFM_LOSS_SQUARE_L2)) return CFFM_ERR_UNSUPPORTED;   // single-process only
    cffm_tables_t view;
    if (B <= 0) return check_shape(s);
    if (!pos || !packed_view(s, packed, n_records, &view)) return CFFM_ERR_UNSUPPORTED;
    const StepCtx c(s, B, theta, ws);
    BwdOpts bo;
    bo.unscaled = true;
    bo.rows = step_rows(&view, pos, s->K + s->D + 4, (int)n_records);
    int rc = backward_impl(c, y, B_global, grad, (hipStream_t)stream, bo);
    return rc ? rc : move_loss_sum(c, grad, (hipStream_t)stream);
}

// the key placement can leave the forward launch when the fused top of the backward runs (and is not the L2 loss path)
static bool defer_rank(const cffm_shape_t* s, int32_t B) {
    return bwd_top_ok(s, B) && s->loss != CFFM_LOSS_SQUARE_L2 && cffm_fwd_all_ok(s, B);
}

extern "C" int cffm_dp_runs_ok(const cffm_shape_t* s, int32_t B) {
    return (check_shape(s) == 0 && B > 0 && cffm_fwd_all_ok(s, B)) ? 1 : 0;
}

// Local half of a data-parallel step in one call: forward (one launch at the README shapes), backward with
// dL/dout = (out - y) / B_global, then slab reduction ∥ row packing.  Same outputs as cffm_forward + cffm_backward_unscaled.
extern "C" int cffm_dp_local(const cffm_shape_t* s, const cffm_tables_t* tab, const float* theta, const int32_t* ids,
                             const float* y, int32_t B, int64_t B_global, void* ws, float* grad, float* rows, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    const StepCtx c(s, B, theta, ws);
    if (!y || s->loss == CFFM_LOSS_HYBRID || s->loss == CFFM_LOSS_SQUARE_L2) return CFFM_ERR_UNSUPPORTED;
    const bool run = cffm_fwd_all_ok(s, B);          // the single-launch forward also leaves this rank's keys sorted; false for a
    const bool later = run && defer_rank(s, B);      // disabled branch: plain forward, no sorted run
    FwdOpts fo;
    fo.no_materialise = true;
    rc = run ? cffm_fwd_all_impl(c, tab, ids, y, st, !later) : forward_impl(c, step_rows(tab, ids), y, st, fo);
    if (rc) return rc;
    BwdOpts bo;
    bo.unscaled = true;
    bo.skip_reduce = true;                           // cffm_dp_tail reduces
    if (later) bo.rank_ids = ids;
    if (!run) bo.rows = step_rows(tab, ids);
    if ((rc = backward_impl(c, y, B_global, grad, st, bo))) return rc;
    return cffm_dp_tail(c, ids, grad, rows, run, st);
}

// Same local half for the dense-table exchange (small vocabularies): flat = [theta gradients | loss sum | table gradient
// image], cffm_dp_dense_floats(s) floats, to be summed over the ranks by ONE all-reduce and handed to cffm_dp_apply_dense.
extern "C" int cffm_dp_local_dense(const cffm_shape_t* s, const cffm_tables_t* tab, const float* theta, const int32_t* ids,
                                   const float* y, int32_t B, int64_t B_global, void* ws, float* flat, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    const StepCtx c(s, B, theta, ws);
    if (!y || s->loss == CFFM_LOSS_HYBRID || s->loss == CFFM_LOSS_SQUARE_L2 || !cffm_fwd_all_ok(s, B)) return CFFM_ERR_UNSUPPORTED;
    // The table image of `flat` must be all zeros on entry: cffm_dp_apply_dense leaves it that way (zero on exit), so only
    // the very first step needs a cleared buffer (the round-2 code paid a hipMemsetAsync of the 1.4 MB image, 4.5 us in front of
    // the forward launch, on every step).
    const bool later = defer_rank(s, B);
    rc = cffm_fwd_all_impl(c, tab, ids, y, st, !later);
    if (rc) return rc;
    BwdOpts bo;
    bo.unscaled = true;
    bo.skip_reduce = true;                           // cffm_dp_tail_dense reduces
    if (later) bo.rank_ids = ids;
    if ((rc = backward_impl(c, y, B_global, flat, st, bo))) return rc;
    return cffm_dp_tail_dense(c, flat, st);
}

extern "C" int cffm_train_step(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* tab_acc,
                               float* theta, float* theta_acc, float* grad, const int32_t* ids, const float* y,
                               int32_t B, void* ws, float* loss, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = check_shape(s);
    if (rc || B <= 0) return rc;
    const StepCtx c(s, B, theta, ws);
    FwdOpts fo;
    fo.fused_step = true;
    BwdOpts bo;
    bo.adagrad_theta = theta; bo.adagrad_acc = theta_acc;    // Adagrad of theta folded into the slab reduction
    bo.loss_out = loss;
    if (s->loss == CFFM_LOSS_SQUARE_L2) {       // regularised square loss: dense table gradients and updates
        // the reference cannot build this graph with a disabled branch either: create_loss reads self.weights['inner_embeddings']
        // and ['outer_embeddings'] (CFFM.py:489-491), which initialize_variables only creates for an enabled branch (:255, :262)
        if (!s->inner_conv || !s->outer_conv) return CFFM_ERR_UNSUPPORTED;
        if ((rc = forward_impl(c, step_rows(tab, ids), y, st, fo))) return rc;
        if ((rc = backward_impl(c, y, (int64_t)B, grad, st, bo))) return rc;
        return cffm_tables_adagrad_l2(c, tab, tab_acc, (int64_t)B * s->F, st);
    }
    if (cffm_fwd_all_ok(s, B)) {                 // small-channel shapes: the whole forward (and the key sort) in one launch
        const bool later = defer_rank(s, B);
        if ((rc = cffm_fwd_all_impl(c, tab, ids, y, st, !later))) return rc;
        bo.skip_reduce = true;                   // cffm_update_all reduces
        if (later) bo.rank_ids = ids;
        if ((rc = backward_impl(c, y, (int64_t)B, grad, st, bo))) return rc;
        return cffm_update_all(c, tab, tab_acc, theta, theta_acc, grad, st);
    }
    fo.no_materialise = true;
    if ((rc = forward_impl(c, step_rows(tab, ids), y, st, fo))) return rc;
    bo.rows = step_rows(tab, ids);
    if ((rc = backward_impl(c, y, (int64_t)B, grad, st, bo))) return rc;
    SortOpts so;
    so.prepacked = true;                         // the gather left the packed keys in ws.sort_keys
    if ((rc = cffm_sort_keys_impl(c, ids, (int64_t)B * s->F, so, st))) return rc;
    return cffm_sparse_apply(c, tab, tab_acc, (int64_t)B * s->F, RowGrads::of_ws(c), LateScale::none(), st);
}

// Where the list step runs in the fused launches: the fused top of the backward, whose key role then places the update's sort keys
// (bwd_top_ok means F <= 11 and B <= 256: within what that role takes, F <= RANK_MAXF and B * F <= 4096), and update_all (Adagrad, both
// branches on: part of bwd_top_ok).  The forward is the single launch where cffm_fwd_all_ok and the stage launches elsewhere (D = 8 or
// 16, and F = 11 at D = 32, whose layer-0 tiles pass the LDS of a CU).  That second combination - stage forward, fused top with the key role, update_all - is this entry point's own: cffm_train_step
// at those shapes takes the folded Adagrad reduction, the sort and cffm_sparse_apply.  It is served because each of the three takes the
// shape on its own terms (the key role asks for F <= RANK_MAXF and B * F <= 4096, update_all for the placed keys and the slabs), and
// tests/test_gpu_list_step.py runs whole steps on it (f4-d8, and f11-d32 with the Pp = 64 top) next to the single-launch forward at f10-d32.  Not the
// regularised loss (dense table updates, stage backward) and not the log loss (its forward leaves sigmoid(out), not the score a list
// loss ranks).
extern "C" int cffm_list_step_ok(const cffm_shape_t* s, int32_t B) {
    if (check_shape(s) || B < 1) return 0;
    return (bwd_top_ok(s, B) && s->optimizer == CFFM_OPT_ADAGRAD && s->loss != CFFM_LOSS_SQUARE_L2 && s->loss != CFFM_LOSS_LOG) ? 1 : 0;
}

// One Adagrad step on G ranked lists of Lg candidates in the launches of cffm_train_step at B = G * Lg (include/cffm_hip.h): id rows,
// forward without labels, list loss on ws.out, backward from its dL/dout through the fused top, update.
// The corrected step (logq: cffm_train_step_lists_logq) differs in the loss call and in the refusals that belong to its three operands.
static int train_step_lists_impl(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* tab_acc, float* theta,
                                 float* theta_acc, float* grad, const int32_t* ctx, int32_t G, const int32_t* fields, int32_t nf,
                                 const int32_t* cand, int64_t cand_stride, int32_t Lg, const int32_t* target, int32_t kind,
                                 int32_t* ids_out, float* dout, float* terms, void* ws, float* loss, void* scratch, bool logq,
                                 const int32_t* lists, const float* corr, int32_t U, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = check_shape(s);
    if (rc || G <= 0) return rc;
    if (Lg < 2 || (kind != CFFM_LIST_BPR && kind != CFFM_LIST_SOFTMAX)) return CFFM_ERR_BAD_SHAPE;
    if (logq && kind == CFFM_LIST_BPR) return CFFM_ERR_UNSUPPORTED;
    const int64_t B64 = (int64_t)G * Lg;
    if (B64 > 0x7fffffff || !cffm_list_step_ok(s, (int32_t)B64)) return CFFM_ERR_UNSUPPORTED;
    const int32_t B = (int32_t)B64;
    if (!tab || !tab_acc || !theta || !theta_acc || !grad || !ctx || !fields || !cand || !target || !ids_out || !dout || !terms || !ws ||
        !loss || !scratch)
        return CFFM_ERR_BAD_SHAPE;
    if (logq && (U < 1 || !lists || !corr || ((uintptr_t)corr & 7))) return CFFM_ERR_BAD_SHAPE;
    const StepCtx c(s, B, theta, ws);
    if ((rc = cffm_route_check(c))) return rc;       // what the forward and the backward ask first: here ahead of the expansion
    // the expansion checks fields / strides itself, before its launch, which is the first of the step
    if ((rc = cffm_expand_candidates_ex(s, ctx, G, fields, nf, cand, cand_stride, Lg, 0, B, ids_out, stream))) return rc;
    // The keys: in the single-launch forward or deferred to the fused top, as cffm_train_step decides (defer_rank - always deferred
    // here, since bwd_top_ok holds); the stage forward places none, so the fused top does there too.
    const bool fwd_all = cffm_fwd_all_ok(s, B), keys_in_fwd = fwd_all && !defer_rank(s, B);
    if (fwd_all) {
        rc = cffm_fwd_all_impl(c, tab, ids_out, nullptr, st, keys_in_fwd);
    } else {
        FwdOpts fo;
        fo.fused_step = true;                        // the inner-branch kernel gathers the rows itself, as in cffm_train_step
        rc = forward_impl(c, step_rows(tab, ids_out), nullptr, st, fo);
    }
    if (rc) return rc;
    const float* out = c.at<const float>(c.wl.out);
    rc = logq ? cffm_list_loss_logq(kind, out, G, Lg, target, lists, corr, U, dout, terms, loss, scratch, stream)
              : cffm_list_loss(kind, out, G, Lg, target, dout, terms, loss, scratch, stream);
    if (rc) return rc;
    BwdOpts bo;
    bo.dout_fused = dout;
    bo.skip_reduce = true;                           // cffm_update_all reduces
    if (!keys_in_fwd) bo.rank_ids = ids_out;
    if ((rc = backward_impl(c, nullptr, (int64_t)B, grad, st, bo))) return rc;
    return cffm_update_all(c, tab, tab_acc, theta, theta_acc, grad, st);
}

extern "C" int cffm_train_step_lists(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* tab_acc, float* theta,
                                     float* theta_acc, float* grad, const int32_t* ctx, int32_t G, const int32_t* fields, int32_t nf,
                                     const int32_t* cand, int64_t cand_stride, int32_t Lg, const int32_t* target, int32_t kind,
                                     int32_t* ids_out, float* dout, float* terms, void* ws, float* loss, void* scratch, void* stream) {
    return train_step_lists_impl(s, tab, tab_acc, theta, theta_acc, grad, ctx, G, fields, nf, cand, cand_stride, Lg, target, kind, ids_out,
                                 dout, terms, ws, loss, scratch, false, nullptr, nullptr, 0, stream);
}

// cffm_train_step_lists with the logQ-corrected softmax as its loss (include/cffm_hip.h): the same launches
extern "C" int cffm_train_step_lists_logq(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* tab_acc, float* theta,
                                          float* theta_acc, float* grad, const int32_t* ctx, int32_t G, const int32_t* fields,
                                          int32_t nf, const int32_t* cand, int64_t cand_stride, int32_t Lg, const int32_t* target,
                                          int32_t kind, int32_t* ids_out, float* dout, float* terms, void* ws, float* loss,
                                          void* scratch, const int32_t* lists, const float* corr, int32_t U, void* stream) {
    return train_step_lists_impl(s, tab, tab_acc, theta, theta_acc, grad, ctx, G, fields, nf, cand, cand_stride, Lg, target, kind, ids_out,
                                 dout, terms, ws, loss, scratch, true, lists, corr, U, stream);
}

extern "C" int cffm_train_step_opt(const cffm_shape_t* s, const cffm_tables_t* tab, const cffm_tables_t* tab_state1,
                                   const cffm_tables_t* tab_state2, float* theta, float* theta_state1, float* theta_state2,
                                   float* grad, const int32_t* ids, const float* y, int32_t B, void* ws, float* loss,
                                   int64_t step, void* stream) {
    int rc = check_shape(s);
    if (rc) return rc;
    if (s->optimizer == CFFM_OPT_ADAGRAD)
        return cffm_train_step(s, tab, tab_state1, theta, theta_state1, grad, ids, y, B, ws, loss, stream);
    if (B <= 0) return 0;
    if (s->loss == CFFM_LOSS_SQUARE_L2 && (!s->inner_conv || !s->outer_conv)) return CFFM_ERR_UNSUPPORTED;   // as in cffm_train_step
    hipStream_t st = (hipStream_t)stream;
    const StepCtx c(s, B, theta, ws);
    FwdOpts fo;
    fo.fused_step = true;
    fo.no_materialise = s->loss != CFFM_LOSS_SQUARE_L2;  // the regularised loss sweeps the tables densely: keep its path as it was
    if ((rc = forward_impl(c, step_rows(tab, ids), y, st, fo))) return rc;
    BwdOpts bo;                                          // gradients only (no fused Adagrad); the loss is written by head_bwd
    bo.loss_out = loss;
    if (fo.no_materialise) bo.rows = step_rows(tab, ids);
    if ((rc = backward_impl(c, y, (int64_t)B, grad, st, bo))) return rc;
    return cffm_apply_opt(c, tab, tab_state1, tab_state2, theta, theta_state1, theta_state2, grad, (int64_t)B * s->F, step, st);
}

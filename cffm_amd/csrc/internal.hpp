// Internal (non-ABI) variants used by the fused composites in api.hip.
#pragma once
#include "common.hpp"

// gather that also emits the sort keys of the sparse update: keys[slot] = (id << 32) | slot
int cffm_gather_impl(const cffm_shape_t* s, const cffm_tables_t* t, const int32_t* ids, int32_t B, float* Ei, float* Eo,
                     float* fb, unsigned long long* keys, hipStream_t st);
// ---- one context per ABI call: what every launch of a step derives from (s, B, theta, ws) ----------------------------------
// Built once by the entry point (shape checked, B >= 1; the update entry points, whose workspace is sized by B_ws, build it with B_ws)
// and handed down: nothing below an entry point derives a layout or a slab plan again.  The builders return complete, value-initialised
// argument blocks, every optional member decided there and nowhere else: conv_args / dgrad_args / wgrad_args of layer l (conv.hip),
// head_args / head_bwd_args (head.hip), inner_fwd_args / inner_bwd_args (inner.hip), sparse_args (optim.hip).
struct ConvArgs; struct DgradArgs; struct WgradArgs; struct HeadArgs; struct HeadBwdArgs; struct InnerFwdArgs; struct InnerBwdArgs;
struct SparseArgs; struct BwdOpts; struct RowGrads;
// late 1/L of the data-parallel step (optim.hip); on == 0: none
struct LateScale {
    const float* sum; float inv_Bg; int on;
    static LateScale none() { return {nullptr, 0.f, 0}; }
};
int cffm_ws_layout_from(const cffm_shape_t* s, int32_t B, const cffm_theta_layout_t& tl, const SlabPlan& sp, cffm_ws_layout_t* out);
struct StepCtx {
    const cffm_shape_t* s;
    int32_t B;
    const float* theta;
    char* w;                     // workspace base
    Geo g;
    cffm_theta_layout_t tl;
    cffm_ws_layout_t wl;
    SlabPlan sp;
    StepCtx(const cffm_shape_t* s_, int32_t B_, const float* theta_, void* ws) : s(s_), B(B_), theta(theta_), w((char*)ws), g(make_geo(s_)) {
        cffm_theta_layout(s, &tl);
        make_slab_plan(s, B, tl, &sp);
        cffm_ws_layout_from(s, B, tl, sp, &wl);
    }
    template <class T = float> T* at(int64_t off) const { return reinterpret_cast<T*>(w + off); }
    const SlabRange& conv_slab(int l) const { return sp.r[sp.conv0 + l]; }
    ConvArgs conv_args(int l) const;
    DgradArgs dgrad_args(int l) const;
    WgradArgs wgrad_args(int l) const;
    // s0_ready: ws.t1[:, 0:D] already holds the s0 pool (the fused gather computed it): ws.Eo is not read
    HeadArgs head_args(const float* y, bool s0_ready = false) const;
    HeadBwdArgs head_bwd_args(const float* y, int64_t B_global, const BwdOpts& o) const;
    // tab != nullptr: the kernel gathers the rows of its example itself (all three tables) and leaves Ei / Eo / fb and the packed sort
    // keys in the workspace
    InnerFwdArgs inner_fwd_args(const cffm_tables_t* tab = nullptr, const int32_t* ids = nullptr) const;
    InnerBwdArgs inner_bwd_args(int* nslab) const;       // *nslab: slabs of the inner range (= workgroups of the kernel)
    // the segment walk over the n_rows sorted keys in ws.sort_vals, row gradients at r
    SparseArgs sparse_args(int64_t n_rows, const RowGrads& r) const;
};
// The per-slot row gradients a table update or a packing kernel reads.  dEi / dEo == NULL: that branch is disabled (CFFM.py:301,
// :348) - it has no table, nothing is applied and its columns travel as zeros.  s*: floats between consecutive slots.
struct RowGrads {
    const float *dEi, *dEo, *dfb;
    int64_t sEi, sEo, sfb;
    static RowGrads of_ws(const StepCtx& c) {            // what the backward left in this context's workspace
        return {c.s->inner_conv ? c.at<const float>(c.wl.dEi) : nullptr, c.s->outer_conv ? c.at<const float>(c.wl.dEo) : nullptr,
                c.at<const float>(c.wl.dfb), c.s->K, c.s->D, 1};
    }
    static RowGrads packed(const cffm_shape_t* s, const float* rows, int64_t W) {    // rows [n][W] = (id bits | dEi | dEo | dfb ...)
        return {s->inner_conv ? rows + 1 : nullptr, s->outer_conv ? rows + 1 + s->K : nullptr, rows + 1 + s->K + s->D, W, W, W};
    }
};
// wide shapes whose forward did not materialise Ei / Eo: the tables (or, stride / records > 0, the packed records) the backward
// re-reads its rows from
struct RowTables {
    const cffm_tables_t* tab = nullptr;
    const int32_t* ids = nullptr;
    int stride = 0, records = 0;
};
struct BwdOpts {
    float* adagrad_theta = nullptr;      // both non-NULL (single-GPU step): the dense Adagrad update is folded into the slab
    float* adagrad_acc = nullptr;        // reduction, and the loss is summed locally
    float* loss_out = nullptr;           // non-NULL: the loss is written here (and summed locally)
    bool local_sum() const { return adagrad_theta != nullptr || loss_out != nullptr; }
    bool unscaled = false;               // data-parallel: dL/dout without the 1/L of the RMSE-style loss
    bool skip_reduce = false;            // the caller reduces the slabs together with the table update
    const int32_t* rank_ids = nullptr;   // non-NULL: the fused top also places the sort keys the forward left out
    const float* dout_in = nullptr;      // non-NULL: device [B], the caller's dL/dout used as given (cffm_backward_dout): the stage route
                                         // at every shape and B, head_bwd_dout_kernel in place of head_bwd_kernel; y is not read
    const float* dout_fused = nullptr;   // non-NULL: device [B], the caller's dL/dout used as given on the FUSED route (bwd_top_ok(s, B)
                                         // and not the regularised loss, else refused): the launches cffm_backward takes there, the fused
                                         // top as its DOUT instance (cffm_backward_dout_fused, cffm_train_step_lists); y is not read
    RowTables rows;
};
struct ConvBwdOpts {
    bool* carry_inner = nullptr;         // non-NULL: a paired launch may carry the inner-branch backward; *carry_inner = true if it did
    bool with_top_wgrad = false;         // the fused top left its weight gradients to this launch (top_wgrad_deferred)
    const RowSrc* rs = nullptr;          // layer 0 of the wide shapes: rows straight from the table
};
// Shapes the shape check accepts but a CU's LDS cannot hold are refused on the host with CFFM_ERR_UNSUPPORTED, before
// anything is launched: check_lds (common.hpp: the inner branch, sized by F * K) and cffm_conv_lds_check (conv.hip: the layer-0
// instance the dispatch picks at this B, sized by F * D).  forward_impl / backward_impl / cffm_fwd_all_impl ask both first, the stage
// launchers ask for their own kernels.
int cffm_conv_lds_check(const StepCtx& c);
static inline int cffm_route_check(const StepCtx& c) {
    const int rc = check_lds(c.s);
    return rc ? rc : cffm_conv_lds_check(c);
}
// forward / backward of conv layer l (0 = the outer-product layer); the exported per-stage entry points wrap these
int cffm_conv_fwd_impl(const StepCtx& c, int l, hipStream_t st, const RowSrc* rs = nullptr);
int cffm_conv_bwd_impl(const StepCtx& c, int l, hipStream_t st, const ConvBwdOpts& o = ConvBwdOpts());
// fused top of the backward (bwd_top_ok(s, B)): head + top conv layers + inner branch in one launch; *next_layer receives the
// highest conv layer the caller still has to run
int cffm_bwd_top_impl(const StepCtx& c, const float* y, int64_t B_global, const BwdOpts& o, hipStream_t st, int* next_layer);
// bwd_fused01_ok: layers 3..0 below the fused top in one launch
int cffm_conv01_bwd_impl(const StepCtx& c, hipStream_t st);
// the head (head.hip).  sum_loss = false skips the separate loss-sum launch (the head backward then sums the terms itself)
struct HeadFwdOpts {
    bool sum_loss = true;
    bool s0_ready = false;               // see StepCtx::head_args
};
int cffm_head_fwd_impl(const StepCtx& c, const float* y, const HeadFwdOpts& o, hipStream_t st);
int cffm_head_bwd_impl(const StepCtx& c, const float* y, int64_t B_global, const BwdOpts& o, hipStream_t st);
// the inner branch (inner.hip); tab / ids as StepCtx::inner_fwd_args, rs != NULL: the rows come straight from the table
int cffm_inner_fwd_impl(const StepCtx& c, const cffm_tables_t* tab, const int32_t* ids, hipStream_t st);
int cffm_inner_bwd_rows(const StepCtx& c, const RowSrc* rs, hipStream_t st);
// theta != nullptr: the dense Adagrad update is fused into the slab reduction
int cffm_reduce_slabs_impl(const StepCtx& c, float* grad, float* theta, float* acc, float lr, hipStream_t st);
// fused single-GPU update (both tables branches on): slab reduction + dense Adagrad and the sorted sparse table update
// as two roles of one launch; the keys must already be sorted in ws.sort_vals
int cffm_update_all(const StepCtx& c, const cffm_tables_t* tab, const cffm_tables_t* tab_acc, float* theta, float* theta_acc,
                    float* grad, hipStream_t st);
// the two steps of the sparse update: stable sort of the packed keys (ws.sort_keys -> ws.sort_vals), then the segment-sum + Adagrad
// sweep.  The sort returns early for n_rows <= 0 and refuses n_rows > B * F of its context.
struct SortOpts {
    bool prepacked = false;              // ws.sort_keys already holds the packed keys: ids is not read
    int64_t id_stride = 1;               // ints between consecutive ids (the id column of packed rows)
};
int cffm_sort_keys_impl(const StepCtx& c, const int32_t* ids, int64_t n_rows, const SortOpts& o, hipStream_t st);
int cffm_sparse_apply(const StepCtx& c, const cffm_tables_t* tab, const cffm_tables_t* acc, int64_t n_rows, const RowGrads& r,
                      const LateScale& ls, hipStream_t st);
// slab reduction (gradients only) and the packing of the rows + local loss sum, two roles of one launch
int cffm_dp_tail(const StepCtx& c, const int32_t* ids, float* grad, float* rows, bool with_run, hipStream_t st);
// dense-table variant of cffm_dp_tail: slab reduction ∥ scatter of this rank's summed row gradients into flat
int cffm_dp_tail_dense(const StepCtx& c, float* flat, hipStream_t st);
// rows[slot] = (id bits | dEi | dEo | dfb) of the workspace's row gradients for the all-gather of the data-parallel step; also copies
// the local loss-term sum (scalars[0]) to *sum_dst
int cffm_pack_rows(const StepCtx& c, const int32_t* ids, float* sum_dst, float* rows, hipStream_t st);
// whole forward of the fused step in one launch (+ the key sort); only for shapes cffm_fwd_all_ok() accepts
bool cffm_fwd_all_ok(const cffm_shape_t* s, int32_t B);
int cffm_fwd_all_impl(const StepCtx& c, const cffm_tables_t* tab, const int32_t* ids, const float* y, hipStream_t st,
                      bool rank_keys);
// CFFM_LOSS_SQUARE_L2: tables updated densely with g = scatter(row grads) + lamda * w (feature_bias stays sparse)
int cffm_tables_adagrad_l2(const StepCtx& c, const cffm_tables_t* tab, const cffm_tables_t* acc, int64_t n_rows, hipStream_t st);
// SGD / Momentum / Adam updates of theta and the three tables from grad + the row gradients in ws (CFFM.py:519-529)
int cffm_apply_opt(const StepCtx& c, const cffm_tables_t* tab, const cffm_tables_t* st1, const cffm_tables_t* st2, float* theta,
                   float* th1, float* th2, const float* grad, int64_t n_rows, int64_t step, hipStream_t st);

// ---- wide shapes (Pp > 64): rows consumed where they are fetched, nothing materialised (RowSrc, common.hpp) ---------------
bool cffm_wide_regather_ok(const cffm_shape_t* s);
int64_t cffm_wb3_bytes(int Pp);     // bytes of the pre-split filter image of the bf16x3 conv loops (conv.hip), forward or input gradient
bool cffm_giw_lds_ok();     // the fused gather's LDS addressing assumption holds for every instance (inner.hip; checked on the host)
// tf.nn.embedding_lookup x3 fused with the inner branch, the s0 pool and the first-order inputs: ids -> ws.inner_out,
// ws.t1[:, 0:D] (s0), ws.fb, ws.sort_keys; Ei / Eo are NOT written
// rows.stride > 0: the three "tables" are views into ONE array of records of rows.stride floats (the packed rows a row-sharded rank
// received: tab->inner_emb = records, outer_emb = records + K, feat_bias = records + K + D) with rows.records records; ids = slot -> record
int cffm_gather_inner_fwd_wide(const StepCtx& c, const RowTables& rows, hipStream_t st);

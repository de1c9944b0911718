/*
 * cffm_hip.h - C ABI of libcffm_hip.so: the CFFM convolutional feature-interaction hot path on
 * MI355X (gfx950).
 *
 * The reference (Anony-CFFM/CFFM) has no FFI: its boundary between host loop and tensor runtime is
 * the pair of TensorFlow session calls
 *     loss, opt = sess.run((self.loss, self.optimizer), feed_dict)      CFFM.py:200   (train step)
 *     batch_out = sess.run((self.out), feed_dict)                       CFFM.py:596   (predict)
 * over the graph built by create_inference_convolutional_feature_interaction_FM (CFFM.py:296-453),
 * create_loss (CFFM.py:486-514) and create_optimizer (CFFM.py:517-529).  The entry points below are
 * what a binding for that seam would call instead; each one cites the graph lines it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (torch tensors in this repo) unless
 *     the name ends in _host; nothing is allocated or freed inside the library;
 *   - every call is asynchronous on the given hipStream_t (passed as void*; NULL = default stream);
 *   - return value: 0 on success, otherwise a hipError_t (or CFFM_ERR_*) - cffm_error_string() gives
 *     the text; no global mutable state, safe from one host thread per device;
 *   - all arithmetic is fp32, ids are int32 (CFFM.py:232-235).
 */
#ifndef CFFM_HIP_H
#define CFFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFFM_ABI_VERSION 9
#define CFFM_MAX_LAYERS 8          /* live conv layers = log2(D) - 1 <= 8  (D <= 512)          */
#define CFFM_MAX_FIELDS 64         /* linear-attention softmax runs inside one 64-lane wavefront */
#define CFFM_HEAD_UNITS 32         /* tf.layers.dense(units=32), CFFM.py:409                    */
#define CFFM_NSLAB 64              /* split-K partial slabs of every dense-gradient producer     */

#define CFFM_ERR_BAD_SHAPE 10001
#define CFFM_ERR_UNSUPPORTED 10002

/* activation ids, CFFM.py:132-141 */
enum { CFFM_ACT_RELU = 0, CFFM_ACT_PRELU = 1, CFFM_ACT_ELU = 2, CFFM_ACT_SELU = 3, CFFM_ACT_GELU = 4 };
/* loss ids, CFFM.py:486-514 (square_loss with lamda == 0 is the README default) */
enum { CFFM_LOSS_SQUARE_RMSE = 0, CFFM_LOSS_MSE = 1, CFFM_LOSS_MAE = 2, CFFM_LOSS_LOG = 3,
       CFFM_LOSS_SQUARE_L2 = 4 /* square_loss with lamda > 0: l2_loss + table regularisers, CFFM.py:489-491 */,
       CFFM_LOSS_HYBRID = 5 /* 0.5*l2_loss(y-out) + 0.5*log_loss(out, y) on the RAW out (NaN once out+1e-7 <= 0), CFFM.py:510-513 */ };

/* optimizer ids, CFFM.py:517-529 */
enum { CFFM_OPT_ADAGRAD = 0, CFFM_OPT_SGD = 1, CFFM_OPT_MOMENTUM = 2, CFFM_OPT_ADAM = 3 };

typedef struct cffm_shape {
    int32_t M;            /* features_M                                   CFFM.py:110            */
    int32_t F;            /* num_field                                    CFFM.py:119            */
    int32_t K;            /* inner_dims (even)                            CFFM.py:105            */
    int32_t D;            /* outer_dims (power of two >= 4)               CFFM.py:106            */
    int32_t act;          /* CFFM_ACT_*                                   CFFM.py:132-141        */
    int32_t linear_att;   /* 1: attention first-order term, 0: plain sum  CFFM.py:423-446        */
    int32_t inner_conv;   /* CFFM.py:301                                                         */
    int32_t outer_conv;   /* CFFM.py:348                                                         */
    int32_t loss;         /* CFFM_LOSS_*                                                         */
    float lamda_att;      /* CFFM.py:434                                                         */
    float beta_outer;     /* CFFM.py:414                                                         */
    float lr;             /* CFFM.py:523                                                         */
    float lamda;          /* lamda_bilinear, only used by CFFM_LOSS_SQUARE_L2    CFFM.py:489-491          */
    int32_t optimizer;    /* CFFM_OPT_*                                          CFFM.py:517-529          */
} cffm_shape_t;

/* Offsets (in floats) of the trained dense parameters inside ONE flat fp32 buffer "theta".  The same
 * layout is used for the Adagrad accumulators and for the gradient buffer.  Untrained variables of
 * the reference (outer_W/outer_b, CFFM.py:271-272; the dead last conv layer, CFFM.py:394-396) are not
 * part of theta - the host keeps them only for the '#params' log line. */
typedef struct cffm_theta_layout {
    int64_t n;                              /* total floats                                        */
    int64_t att_W, att_b;                   /* bias_W [F,F], bias_b [F]          CFFM.py:281-282   */
    int64_t bias;                           /* scalar                            CFFM.py:284       */
    int64_t inner_cw, inner_cb;             /* [2 taps][2 ch], [2]               CFFM.py:323       */
    int64_t inner_dw, inner_db;             /* dense [P*K], [1]                  CFFM.py:339       */
    int64_t conv_w[CFFM_MAX_LAYERS];        /* HWIO [2,2,P,P] stored [4][Pp][Pp], zero pads  CFFM.py:375-377 */
    int64_t conv_b[CFFM_MAX_LAYERS];        /* [Pp], zero pads                                     */
    int64_t d1_w, d1_b;                     /* [2D-2][32], [32]                  CFFM.py:409       */
    int64_t d2_w, d2_b;                     /* [32], [1]                         CFFM.py:410       */
    int64_t lin_w, lin_b;                   /* [F], [1]                          CFFM.py:441       */
    int32_t P, Pp, Lc, live;                /* pairs, pairs padded to 16, log2(D), Lc-1            */
} cffm_theta_layout_t;

/* Byte offsets of every intermediate inside the caller-provided workspace for a batch of B rows.
 * Exposed so that the parity tests can read each tensor back and compare it with the oracle. */
typedef struct cffm_ws_layout {
    int64_t bytes;
    int64_t Ei, Eo, fb;                     /* gathered rows [B,F,K] [B,F,D] [B,F]                 */
    int64_t inner_out;                      /* [B]                                                 */
    int64_t C[CFFM_MAX_LAYERS];             /* relu(conv_l + b_l)  [B,S_l,S_l,Pp], S_l = D>>(l+1)  */
    int64_t t1, h1, att, out;               /* [B,2D-2] [B,32] [B,F] [B]                           */
    int64_t sqerr;                          /* per-example loss term [B]                           */
    int64_t scalars;                        /* [0]=sum of loss terms (local) [1]=loss [2]=dscale [3]=sum used */
    int64_t dout, dt1;                      /* [B], [B,2D-2]                                       */
    int64_t dC[CFFM_MAX_LAYERS];            /* grad wrt C_l, same shape as C_l                     */
    int64_t dEi, dEo, dfb;                  /* IndexedSlices values [B,F,K] [B,F,D] [B,F]          */
    int64_t gpart;                          /* split-K partial gradients, per theta range [nslab][len] */
    int64_t gpart_floats;
    int64_t sort_keys, sort_vals;           /* int32 [B*F] each (sorted ids, source slots)         */
    int64_t sort_tmp;                       /* radix sort scratch                                  */
    int64_t sort_tmp_bytes;
    int64_t Gi, Go, Gfb;                    /* dense table gradients [M,K], [M,D], [M] (CFFM_LOSS_SQUARE_L2, CFFM_OPT_ADAM) */
    int64_t pool[CFFM_MAX_LAYERS];          /* wide shapes (Pp > 64): partial sum pools of act(C_l) left by the conv epilogues,
                                               [B][S_l][pool_np[l]] floats (0 = not used); the head adds the partials up       */
    int32_t pool_np[CFFM_MAX_LAYERS];       /* partials per (example, row y) of layer l                                          */
    int64_t w0pack;                         /* wide shapes with the tiled layer 0: the layer-0 filter re-laid out as MFMA operand
                                               fragments for the input-gradient kernel (rebuilt from theta by every backward pass;
                                               0 = not used)                                                                        */
    int64_t w0pack_floats;
    int64_t relu0;                          /* wide shapes with the tiled layer 0: one bit per element of C[0] .. C[live-2], set where
                                               C[l] > 0 (16-bit words, [B*S_l*S_l][Pp/16] per layer, one layer after the other), written
                                               by the forward of layer l and read by the input gradient of layer l+1 instead of C[l]
                                               itself (0 = not used)                                                               */
    int64_t wb3;                            /* wide shapes: scratch for ONE conv filter split into three bf16 pieces in the record order
                                               of the bf16x3 contraction ([k-step][piece][kk][padded column] x 16 bytes; rebuilt in front
                                               of every direct conv forward / input-gradient launch; 0 = not used)                     */
    int64_t wb3_bytes;
} cffm_ws_layout_t;

typedef struct cffm_tables {                /* the three gathered variables and nothing else       */
    float *inner_emb;                       /* [M,K]  inner_embeddings  CFFM.py:257                */
    float *outer_emb;                       /* [M,D]  outer_embeddings  CFFM.py:264                */
    float *feat_bias;                       /* [M]    feature_bias      CFFM.py:276                */
} cffm_tables_t;

/* Which kernel instance runs one role of a conv layer.  family: one of the values below, by role; a member the family's kernel
 * does not have as a template argument is 0. */
#define CFFM_CHOICE_UNSUPPORTED (-1)  /* any role: no kernel is compiled for it, the stage returns CFFM_ERR_UNSUPPORTED          */
#define CFFM_FWD_FACT 1               /* conv0_fact_fwd_kernel<NT>: factorised layer 0 of the narrow filters (Pp <= 64)           */
#define CFFM_FWD_ROWS 2               /* conv_fwd_rows_kernel<NT, RM>: narrow, whole filter in LDS                                 */
#define CFFM_FWD_TAPS 3               /* conv_fwd_taps_kernel<NT, RM>: narrow, one wavefront per filter tap                        */
#define CFFM_FWD_TILE 4               /* conv0_fact_tile_fwd_kernel: tiled factorised layer 0 of the wide filters                  */
#define CFFM_FWD_TILE_PACKED 5        /* conv0_fact_tile_fwd2_kernel: the same on the packed filter (ws.w0pack)                    */
#define CFFM_FWD_DIRECT 6             /* conv_fwd_kernel<NT, RM>: implicit GEMM of the wide filters                                */
#define CFFM_WGRAD_FACT_BWD 1         /* conv0_fact_bwd_kernel<NT>: narrow layer 0, weight, bias AND input gradient (dgrad: NONE)  */
#define CFFM_WGRAD_TAPS 2             /* wgrad_taps_kernel<NT, HALVES>; paired: the weight-gradient role of conv_bwd_pair_kernel   */
#define CFFM_WGRAD_TILE_ALL 3         /* conv0_fact_tile_wgrad_all_kernel: tiled layer 0, all groups in one workgroup              */
#define CFFM_WGRAD_TILE_GROUP 4       /* conv0_fact_tile_wgrad_kernel: tiled layer 0, one workgroup per group (F = 33)             */
#define CFFM_WGRAD_DIRECT0 5          /* wgrad_kernel<NT>: direct layer 0                                                          */
#define CFFM_WGRAD_WGRAD2 6           /* wgrad2_kernel<NT>: layers >= 1 of the wide filters, fp32 MFMA                             */
#define CFFM_WGRAD_WGRAD3 7           /* wgrad3_kernel<NT>: the same tile as bf16x3                                                */
#define CFFM_DGRAD_NONE 0             /* the weight-gradient launch also computes the input gradient (CFFM_WGRAD_FACT_BWD)         */
#define CFFM_DGRAD_TAPS 1             /* dgrad_taps_kernel<NT, RM, HALVES>; paired: the input-gradient role of conv_bwd_pair_kernel */
#define CFFM_DGRAD_TILE_PACKED 2      /* conv0_fact_tile_dgrad2_kernel: tiled layer 0 on the packed filter                         */
#define CFFM_DGRAD_DIRECT 3           /* dgrad_kernel<NT, RM>: implicit GEMM of the wide filters                                   */
typedef struct cffm_kernel_choice {
    int32_t family;
    int32_t NT;                             /* column tiles of 16 channels per workgroup                                       */
    int32_t RM;                             /* row tiles per workgroup: of 16 rows (ROWS: 64) narrow, of 64 rows DIRECT        */
    int32_t HALVES;                         /* 256-thread halves of a tap-split gradient workgroup                             */
    int32_t b3;                             /* 1: bf16x3 contraction on the bf16 pipe; always 0 under CFFM_CONV_FP32=1          */
} cffm_kernel_choice_t;
typedef struct cffm_conv_choice {
    cffm_kernel_choice_t fwd, wgrad, dgrad;
    int32_t paired;                         /* 1: wgrad and dgrad are two roles of ONE launch, conv_bwd_pair_kernel<NT, dgrad.RM> */
    int32_t top_wgrad_deferred;             /* 1: the slab plan of (shape, B) leaves the weight gradients of the fused top of the
                                               backward to the pair launch of the layer below it (the same for every layer)      */
} cffm_conv_choice_t;

/* ---- layout queries (host only, no GPU needed) -------------------------------------------------- */
int cffm_abi_version(void);
const char *cffm_error_string(int err);
int cffm_theta_layout(const cffm_shape_t *s, cffm_theta_layout_t *out);
/* Pure layout queries: they serve every shape the shape check accepts.  What a step can RUN is smaller: with the
 * inner branch on, 5 F K + Pp + 8 floats must fit a CU's LDS (163,328 bytes), and with the outer branch on the layer-0 kernels
 * bound F * D (every F up to D = 64; F <= 48 except 11 at D = 128, F <= 24 at D = 256, F <= 8 or F = 12 at D = 512).  Every entry
 * point that launches returns CFFM_ERR_UNSUPPORTED for a shape beyond that, before anything is launched.  One answer per shape:
 * a forward-only caller is refused too where only a backward kernel does not fit. */
int cffm_ws_layout(const cffm_shape_t *s, int32_t B, cffm_ws_layout_t *out);
/* The kernels cffm_outer_conv0_fwd / cffm_conv_fwd and cffm_outer_conv0_bwd / cffm_conv_bwd launch for conv layer `layer`
 * (0 <= layer < live) of shape s at batch B >= 1, with the slab count of the real slab plan: the one decision the stages
 * themselves switch on.  Launches nothing.  b3 reflects this process's CFFM_CONV_FP32 latch. */
int cffm_conv_choice(const cffm_shape_t *s, int32_t B, int32_t layer, cffm_conv_choice_t *out);
/* Which launches of the fused train step run the instance that has the shape compiled in (the frappe command: F = 10, K = D = 32,
 * selu), as a bit set; 0 for every other shape and wherever (shape, B) does not take that launch at all.  The conv01 bit also needs
 * a loss other than square_l2, as the launch does.  Launches nothing; CFFM_ERR_BAD_SHAPE for a shape the shape check refuses or
 * B < 1.  Additive entry point: CFFM_ABI_VERSION stays 9. */
#define CFFM_FUSED_INSTANCE_FWD 1     /* fwd_all_kernel<3, 16, selu, 10, 32, 32>                                                   */
#define CFFM_FUSED_INSTANCE_BWD_TOP 2 /* reserved for bwd_top_kernel: no compiled-shape instance of it exists, the bit is never set */
#define CFFM_FUSED_INSTANCE_CONV01 4  /* conv01_bwd_kernel<3, 10, 32, selu>                                                        */
int cffm_fused_instance(const cffm_shape_t *s, int32_t B);

/* ---- stage entry points ------------------------------------------------------------------------ */
/* tf.nn.embedding_lookup x3 (CFFM.py:303, :354, :422): ids int32 [B*F] -> Ei [B,F,K], Eo [B,F,D],
 * fb [B,F].  Any of the three outputs may be NULL to skip that table. */
int cffm_gather(const cffm_shape_t *s, const cffm_tables_t *t, const int32_t *ids, int32_t B,
                float *Ei, float *Eo, float *fb, void *stream);

/* The read-only form of the three lookups for WIDE shapes (F*(F-1)/2 > 64, K == D in {32, 64}, F <= 32: BASELINE configs[3]
 * and [4]): tf.nn.embedding_lookup x3 (CFFM.py:303, :354, :422) fused with every consumer of a whole looked-up example - the
 * inner branch (CFFM.py:304-343), the s0 sum pool of the outer-product map (CFFM.py:381) and the first-order inputs
 * (CFFM.py:422): ids [B,F] -> ws.inner_out [B], ws.t1[:, 0:D] (s0), ws.fb [B,F], ws.sort_keys.  The rows go HBM -> LDS ->
 * registers and are NOT written to ws.Ei / ws.Eo (cffm_predict / cffm_train_step / cffm_dp_local then fetch the rows again
 * from the tables in the few later kernels that need them).  This is the kernel the HBM-gather roofline is quoted on.
 * Returns CFFM_ERR_UNSUPPORTED for other shapes (cffm_gather_inner_fwd_ok(s) == 0): those run cffm_gather / the fused
 * small-shape forward. */
int cffm_gather_inner_fwd_ok(const cffm_shape_t *s);
int cffm_gather_inner_fwd(const cffm_shape_t *s, const cffm_tables_t *t, const float *theta, const int32_t *ids, int32_t B,
                          void *ws, void *stream);

/* inner branch CFFM.py:304-343 on gathered rows: ws.Ei -> ws.inner_out */
int cffm_inner_fwd(const cffm_shape_t *s, const float *theta, void *ws, int32_t B, void *stream);
/* its gradient: ws.dout, ws.Ei -> ws.dEi, gpart slabs of inner_cw/inner_cb/inner_dw/inner_db */
int cffm_inner_bwd(const cffm_shape_t *s, const float *theta, void *ws, int32_t B, void *stream);

/* STAGE CONTRACT FOR WIDE SHAPES (Pp = ceil16(F*(F-1)/2) > 64, every activation but gelu).  The forward stages leave two
 * side products in the workspace and the later stages CONSUME THOSE instead of re-reading the conv outputs:
 *   ws.pool[l]   row-sum partials of C[l] (CFFM.py:381, :390) written by the epilogue of cffm_outer_conv0_fwd (l = 0) and
 *                cffm_conv_fwd (l >= 1); cffm_head_fwd sums THESE and does not read ws.C[*];
 *   ws.relu0     relu bit masks of C[0] .. C[live-2], one 16-bit word per (pixel, 16 channels), written by the same
 *                epilogues; cffm_conv_bwd (l >= 1) reads the mask of C[l-1] in place of ws.C[l-1].
 * A caller that writes ws.C itself, or runs another forward on the same workspace between a forward stage and its consumer,
 * must re-run cffm_outer_conv0_fwd / cffm_conv_fwd for that layer first: stale pools / masks are not detected.  The narrow
 * shapes (Pp <= 64) and gelu keep the contract written at each entry point below (pools and masks are swept from ws.C). */
/* outer product fused with conv layer 0 (CFFM.py:355-367 + :385-386 for i = 0): ws.Eo -> ws.C[0] (wide: + ws.pool[0], ws.relu0) */
int cffm_outer_conv0_fwd(const cffm_shape_t *s, const float *theta, void *ws, int32_t B, void *stream);
/* ws.dC[0], ws.dt1, ws.Eo -> ws.dEo, gpart slabs of conv_w[0]/conv_b[0] */
int cffm_outer_conv0_bwd(const cffm_shape_t *s, const float *theta, void *ws, int32_t B, void *stream);

/* conv layer l >= 1 (CFFM.py:385-387): ws.C[l-1] -> ws.C[l] (wide: + ws.pool[l], and the relu mask of C[l] for l <= live-2).
 * Wide shapes (128-channel tiles, >= 32768 rows) contract on the bf16 MFMA pipe at fp32 accuracy (error-free 3-way bf16 split of both
 * operands, six cross terms, fp32 accumulate; ws.wb3 is their scratch); the environment variable CFFM_CONV_FP32=1 selects the fp32 MFMA
 * loops.  The same holds for cffm_conv_bwd (input gradient; its weight gradient at any row count). */
int cffm_conv_fwd(const cffm_shape_t *s, const float *theta, void *ws, int32_t B, int32_t layer, void *stream);
/* ws.dC[l], ws.C[l-1], ws.dt1 -> ws.dC[l-1], gpart slabs of conv_w[l]/conv_b[l].  Wide shapes: the input gradient takes the
 * relu mask of C[l-1] from ws.relu0 (see the stage contract above); the weight gradient still reads ws.C[l-1]. */
int cffm_conv_bwd(const cffm_shape_t *s, const float *theta, void *ws, int32_t B, int32_t layer, void *stream);

/* sum pooling + concat + dense heads + first-order term + add_n (CFFM.py:381, :390-396, :409-453):
 * ws.C[*], ws.Eo, ws.fb, ws.inner_out -> ws.t1, ws.h1, ws.att, ws.out; when y != NULL also ws.sqerr and
 * scalars[0] = sum of per-example loss terms over the B local rows.  Wide shapes: ws.pool[*] in place of ws.C[*] (see the
 * stage contract above). */
int cffm_head_fwd(const cffm_shape_t *s, const float *theta, void *ws, const float *y, int32_t B, void *stream);
/* loss gradient (CFFM.py:493) and the head's backward: ws.out, y, scalars[3] (the loss-term sum over
 * the GLOBAL batch of B_global rows) -> ws.dout, ws.dt1, ws.dfb, ws.dC[live-1], gpart slabs of the
 * head parameters, scalars[1] = loss. */
int cffm_head_bwd(const cffm_shape_t *s, const float *theta, void *ws, const float *y, int32_t B,
                  int64_t B_global, void *stream);

/* sum the split-K slabs of ws.gpart (and the finer x-slabs of conv layer 0) in slab order -> grad [theta.n];
 * bitwise reproducible.  B = the batch size the workspace was laid out for. */
int cffm_reduce_slabs(const cffm_shape_t *s, void *ws, int32_t B, float *grad, void *stream);

/* tf.train.AdagradOptimizer (CFFM.py:523-524), dense: acc += g*g; v -= lr*g/sqrt(acc) over n floats */
int cffm_dense_adagrad(float *theta, float *acc, const float *grad, int64_t n, float lr, void *stream);
/* sparse: ids int32 [n_rows] with row gradients dEi [n_rows,K], dEo [n_rows,D], dfb [n_rows]; duplicate
 * ids are summed FIRST (in slot order), then one update per distinct row; other rows untouched. */
int cffm_sparse_adagrad(const cffm_shape_t *s, const cffm_tables_t *tab, const cffm_tables_t *acc,
                        const int32_t *ids, int64_t n_rows, const float *dEi, const float *dEo,
                        const float *dfb, void *ws, int32_t B_ws, void *stream);

/* ---- composites: what CFFM.evaluate / CFFM.train call in place of the two sess.run()s ------------- */
/* sess.run(self.out) CFFM.py:596: ids [B,F] -> out [B] (also left in ws.out).  Where cffm_train_step runs its forward in one
 * launch (narrow shapes, B * F <= 4096) this runs the same launch: out equals the train step's ws.out on the same ids bit for bit. */
int cffm_predict(const cffm_shape_t *s, const cffm_tables_t *tab, const float *theta, const int32_t *ids,
                 int32_t B, void *ws, float *out, void *stream);
/* forward half of a train step, through the per-example loss terms.  tab == NULL: the looked-up rows are already
 * staged in ws.Ei / ws.Eo / ws.fb (row-sharded tables: they arrived from their owner ranks) and ids is not read */
int cffm_forward(const cffm_shape_t *s, const cffm_tables_t *tab, const float *theta, const int32_t *ids,
                 const float *y, int32_t B, void *ws, void *stream);
/* backward half: needs scalars[3] = global loss-term sum (cffm_train_step copies scalars[0] there) */
int cffm_backward(const cffm_shape_t *s, const float *theta, const float *y, int32_t B, int64_t B_global,
                  void *ws, float *grad, void *stream);
/* cffm_forward + cffm_backward_unscaled in one call (what one rank runs before the two collectives of a
 * data-parallel step); uses the single-launch forward where the shape allows.  rows must hold B*F*(1+K+D+1 + 2) floats:
 * the packed rows [B*F][1+K+D+1] followed by this rank's B*F update keys (id << 32 | slot, 64-bit; an id outside [0, M) is
 * keyed as M, while column 0 of its row keeps the raw bits) in sorted order (a "run"; valid when the single-launch forward ran, i.e. Pp <= 64 and B*F <= 4096) */
/* 1 if cffm_dp_local with this per-rank batch leaves a valid sorted run behind its rows (else pass n_runs = 0 rows) */
int cffm_dp_runs_ok(const cffm_shape_t *s, int32_t B);
int cffm_dp_local(const cffm_shape_t *s, const cffm_tables_t *tab, const float *theta, const int32_t *ids, const float *y,
                  int32_t B, int64_t B_global, void *ws, float *grad, float *rows, void *stream);
/* Dense-table exchange for small vocabularies (M*(K+D+1) floats fewer than all ranks' row gradients): the local half
 * leaves ONE buffer flat = [theta.n gradients | loss sum | pad | duplicates-summed table gradients as a dense
 * [M][K | D | 1] image] of cffm_dp_dense_floats(s) floats; the caller all-reduces (sums) it over the ranks and every
 * rank applies it with cffm_dp_apply_dense (rows nobody looked up carry 0 and stay bit-identical).  Needs the
 * single-launch forward (cffm_dp_runs_ok(s, B)).
 * CONTRACT of the image: all zeros on entry of cffm_dp_local_dense (which only writes the rows this rank looked up), all
 * zeros again on return of cffm_dp_apply_dense (it clears every element it reads).  The caller zeroes the buffer ONCE,
 * when it allocates it, and after any step it abandoned between the two calls. */
int64_t cffm_dp_dense_floats(const cffm_shape_t *s);
int cffm_dp_local_dense(const cffm_shape_t *s, const cffm_tables_t *tab, const float *theta, const int32_t *ids,
                        const float *y, int32_t B, int64_t B_global, void *ws, float *flat, void *stream);
int cffm_dp_apply_dense(const cffm_shape_t *s, const cffm_tables_t *tab, const cffm_tables_t *acc, float *theta,
                        float *theta_acc, float *flat_sum, int64_t B_global, float *loss_out, void *stream);
/* Data-parallel halves (cffm_amd/dist.py).  cffm_backward_unscaled = cffm_backward with dL/dout = (out - y) / B_global,
 * i.e. without the 1/L of the RMSE-style loss (CFFM.py:493), which needs the loss-term sum over the GLOBAL batch:
 * grad must hold theta.n + 4 floats, grad[theta.n] receives this rank's loss-term sum so that one all-reduce carries
 * gradients and sum; rows [B*F][1+K+D+1] receives (id bits | dEi | dEo | dfb) for one all-gather.  cffm_dp_apply with
 * n_runs = 0 takes rows [n_rows][1+K+D+1] in any order and sorts the keys itself; with n_runs > 0 rows is the
 * concatenation of n_runs cffm_dp_local buffers (n_rows / n_runs slots each): the sorted runs are merged by rank
 * (binary searches in LDS) instead of a radix sort of all n_rows keys.  cffm_dp_apply takes
 * the all-reduced grad and the all-gathered rows, applies 1/L and the dense + sparse Adagrad updates.  These two entry
 * points (cffm_dp_apply, cffm_dp_apply_dense) are Adagrad only: any other s->optimizer returns CFFM_ERR_UNSUPPORTED
 * before a pointer is read.  cffm_dp_apply_opt (below) is the apply of the other optimizers. */
int cffm_backward_unscaled(const cffm_shape_t *s, const float *theta, const int32_t *ids, const float *y, int32_t B,
                           int64_t B_global, void *ws, float *grad, float *rows, void *stream);
int cffm_dp_apply(const cffm_shape_t *s, const cffm_tables_t *tab, const cffm_tables_t *acc, float *theta,
                  float *theta_acc, const float *grad_sum, int64_t B_global, const float *rows, int64_t n_rows,
                  void *ws, int32_t B_ws, float *loss_out, int32_t n_runs, void *stream);
/* cffm_dp_apply for every optimizer the multi-GPU steps run (as cffm_train_step_opt is to cffm_train_step): the same
 * arguments, the same three routes (sorted runs merged, <= 8192 keys placed, else radix sort) and the same late 1/L.
 * CFFM_OPT_ADAGRAD forwards to cffm_dp_apply.  CFFM_OPT_SGD: w -= lr * g.  CFFM_OPT_MOMENTUM: a = 0.95 * a + g, w -= lr * a,
 * with acc / theta_acc read as the Momentum accumulators (the first slot; both may be NULL for SGD).  theta gets the dense
 * rule; a table row gets the rule once, on the sum of its duplicates, and only if some rank looked it up: the other rows
 * and their accumulators are neither read nor written (TF's sparse apply; an untouched row's accumulator does not decay).
 * CFFM_OPT_ADAM returns CFFM_ERR_UNSUPPORTED right after the shape check, before a pointer is read: TF's sparse Adam is
 * non-lazy (every row of every table moves every step), which is a dense sweep and not this exchange.  There is no
 * dense-image variant (cffm_dp_apply_dense stays Adagrad only): an exact 0 in the all-reduced image cannot tell "row not
 * looked up" from "gradients summed to 0", and Momentum must decay the accumulator in the second case only.
 * CFFM_ERR_BAD_SHAPE as cffm_dp_apply (n_rows / n_runs / B_ws), checked before the first launch. */
int cffm_dp_apply_opt(const cffm_shape_t *s, const cffm_tables_t *tab, const cffm_tables_t *acc, float *theta,
                      float *theta_acc, const float *grad_sum, int64_t B_global, const float *rows, int64_t n_rows,
                      void *ws, int32_t B_ws, float *loss_out, int32_t n_runs, void *stream);
/* sess.run((self.loss, self.optimizer)) CFFM.py:200: one fused forward + backward + Adagrad update of
 * theta/tables (and their accumulators) in place; loss (device scalar, may be NULL) receives the loss. */
int cffm_train_step(const cffm_shape_t *s, const cffm_tables_t *tab, const cffm_tables_t *tab_acc,
                    float *theta, float *theta_acc, float *grad, const int32_t *ids, const float *y,
                    int32_t B, void *ws, float *loss, void *stream);

/* ---- row-sharded tables (cffm_amd/dist.py ShardedStep) -------------------------------------------------
 * The reference is single-device: these replace nothing in it; they are the device side of the three all-to-alls.
 * A looked-up row travels as ONE packed record of cffm_packed_row_floats(s) = K + D + 4 floats:
 * (inner row | outer row | feature_bias, 0, 0, 0), i.e. tf.nn.embedding_lookup x3 (CFFM.py:303, :354, :422) of one id. */
int32_t cffm_packed_row_floats(const cffm_shape_t *s);
/* owner side: rows int32 [n] (local row indices) -> out [n][K+D+4] */
int cffm_gather_packed(const cffm_shape_t *s, const cffm_tables_t *t, const int32_t *rows, int64_t n, float *out, void *stream);
/* requester side: slot i of the [B,F] batch takes record pos[i] of packed [n_records][K+D+4] (pos == NULL: record i) ->
 * ws.Ei / ws.Eo / ws.fb, ready for cffm_forward(tab = NULL) */
int cffm_stage_packed(const cffm_shape_t *s, const float *packed, const int32_t *pos, int64_t n_records, int32_t B, void *ws,
                      void *stream);
/* The same two halves WITHOUT staging, for the wide shapes (cffm_gather_inner_fwd_ok(s); CFFM_ERR_UNSUPPORTED otherwise - use
 * cffm_stage_packed + cffm_forward(tab = NULL) + cffm_backward_unscaled there): the records are consumed where they lie - slot i reads
 * record pos[i] in the kernel that fetches it (cffm_gather_inner_fwd_wide with a record stride), the later kernels that need a row again
 * read it from the records - so ws.Ei / ws.Eo are never written, exactly as cffm_predict / cffm_train_step run on replicated tables.
 * cffm_backward_unscaled_packed leaves ws.dEi / ws.dEo / ws.dfb for cffm_pack_rows_dedup and this rank's loss-term sum in grad[theta.n]. */
int cffm_forward_packed(const cffm_shape_t *s, const float *theta, const float *packed, const int32_t *pos, int64_t n_records,
                        const float *y, int32_t B, void *ws, void *stream);
int cffm_backward_unscaled_packed(const cffm_shape_t *s, const float *theta, const float *packed, const int32_t *pos,
                                  int64_t n_records, const float *y, int32_t B, int64_t B_global, void *ws, float *grad, void *stream);
/* gradient message with the duplicates of one id summed first, in slot order: order int32 [B*F] = slot at sorted position q
 * (sorted by destination, stable), uniq int32 [B*F] = index of the distinct id at position q (non-decreasing), local_ids
 * int32 [B*F] = the owner's row of every slot; ws.dEi / ws.dEo / ws.dfb -> out [#distinct][1+K+D+1] = (row bits | dEi |
 * dEo | dfb), the row format cffm_dp_apply takes */
int cffm_pack_rows_dedup(const cffm_shape_t *s, const int32_t *local_ids, const int32_t *order, const int32_t *uniq, int32_t B,
                         void *ws, float *out, void *stream);

/* routing plan of one [B,F] batch (n = B*F slots) through tables of M global rows sharded r -> (rank r % world, local row r / world);
 * a function of the ids alone, so ShardedStep issues it one step ahead.  All outputs int32 [n] except counts int64 [world]:
 *   local_ids  owner's local row of every slot                       order  slot at sorted position q ((owner, local row) order,
 *   uniq       index of the distinct (owner, local row) pair at q           stable: slots ascend inside a run of equal ids)
 *   pos        slot -> index of its distinct pair                    send_rows  local row of distinct pair u (first #distinct used)
 *   counts     distinct pairs per owner = the split sizes of the three all-to-alls (summed: #distinct)
 * = what cffm_pack_rows_dedup / cffm_stage_packed take.  scratch: cffm_shard_plan_scratch_bytes(n) bytes.  ids must lie in [0, M). */
int64_t cffm_shard_plan_scratch_bytes(int64_t n);
int cffm_shard_plan(const int32_t *ids, int64_t n, int32_t world, int64_t M, void *scratch, int32_t *local_ids, int32_t *order,
                    int32_t *uniq, int32_t *pos, int32_t *send_rows, int64_t *counts, void *stream);

/* ---- tables drawn by GLOBAL row (HipEngine(params='device_rows'); cffm_amd/spec.py table_rows is the numpy twin) ---
 * Additive entry point: CFFM_ABI_VERSION stays 9, no existing signature or struct changes.
 * Local row l (0 <= l < n_rows <= s->M) of the tables holds GLOBAL row g = row0 + l * row_step, and a value depends on
 * (seed, g, table, column) alone: rank r of G draws its shard with (row0, row_step) = (r, G), one process with (0, 1), and
 * the shards of any world size are rows of the same model.  The generator:
 *   block cipher  Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85
 *   key           (seed & 0xffffffff, seed >> 32)
 *   counter       (g & 0xffffffff, g >> 32, q, t): q = index of a group of four columns, t = 0 inner_embeddings, 1 outer_embeddings
 *   uniforms      output words x0..x3 -> columns 4q..4q+3:  u1 = ((x0 >> 8) + 1) * 2^-24, u2 = (x1 >> 8) * 2^-24,
 *                 r = sqrt(-2 ln u1), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2); z2, z3 likewise from x2, x3
 *   stored value  0.1 * z (inner, CFFM.py:257), 0.01 * z (outer, CFFM.py:264), feat_bias exact 0 (CFFM.py:276)
 * Columns >= K or >= D are dropped (K and D only have to be even here); the table of a disabled branch is not written; a NULL
 * feat_bias is skipped.  CFFM_ERR_BAD_SHAPE for row0 < 0, row_step < 1, n_rows < 0, n_rows > s->M, a last global row beyond
 * int64, a NULL (or not 8-byte aligned) table of an enabled branch - before anything is launched; n_rows == 0 returns 0
 * without a launch.  Optimizer slots are the caller's business. */
int cffm_init_table_rows(const cffm_shape_t *s, const cffm_tables_t *tab, uint64_t seed, int64_t row0, int64_t row_step,
                         int64_t n_rows, void *stream);

/* ---- evaluate() (CFFM.py:583-615) without a device-to-host copy of the predictions ------------------------------- */
/* clip + metric sums of CFFM.py:607-614 over n rows: p = min(max(pred, lo), hi) with lo/hi = min/max of the split's labels;
 * sums[0] += sum (y - p)^2, sums[1] += sum y, sums[2] += sum y^2, all float64, in a fixed order (bitwise reproducible).
 * sums is ACCUMULATED so that a split swept in several blocks of rows adds up (zero it first); scratch must hold
 * cffm_eval_scratch_bytes() bytes.  RMSE = sqrt(sums[0]/N), R2 = 1 - sums[0] / (sums[2] - sums[1]^2/N). */
int64_t cffm_eval_scratch_bytes(void);
int cffm_eval_sums(const float *pred, const float *y, int64_t n, float lo, float hi, void *scratch, double *sums,
                   void *stream);

/* ---- candidate ranking: score, top-k and rank-of-target on the device (cffm_amd/csrc/rank.hip) ---------------------
 * Additive entry points: CFFM_ABI_VERSION stays 9, no existing signature, struct or kernel changes.  The reference has no
 * ranking sweep (its evaluate() stops at RMSE / R2, CFFM.py:583-615): these replace nothing in it.
 * THE ORDER on the candidates of one context, used by cffm_topk, cffm_rank_of and the numpy reference of the tests alike:
 *   scores compare as IEEE floats with -0 == +0; NaN ranks below everything, -inf included; among equal scores the smaller
 *   candidate position wins.  As a 64-bit key (larger = better): u = bits(s + 0.0f); key32 = 0 if s is NaN, ~u if the sign bit
 *   of u is set, else u | 0x80000000; key64 = key32 << 32 | (0xffffffff - position); a skipped candidate has key64 = 0.
 * Every compare is a 64-bit integer compare: the results are the same bits on every run.
 * Argument rules: scores is [C][row_stride] floats with row_stride >= N, elements beyond N of a row are never read; skip may be
 * NULL, else [C][skip_stride] bytes, non-zero = skipped.  C == 0 (rows == 0) returns 0 without a launch.  CFFM_ERR_BAD_SHAPE,
 * before the first launch or HIP call, for: a NULL pointer that would be read or written; field outside [0, F); N < 1; k < 1;
 * k > 1024; first < 0; rows < 0; first + rows > C * N; row_stride < N; skip_stride < N with skip != NULL.
 *
 * cffm_expand_candidates: the id rows of (context, candidate) pairs.  For global row g in [first, first + rows) of the flattened
 * [C * N] range, c = g / N, n = g % N: ids_out[g - first][f] = (f == field) ? cand[n] : ctx[c][f]; ctx int32 [C][F], cand int32 [N].
 * Writes exactly rows * F int32 values and nothing else.  Ids are not validated: cffm_predict clamps them as it always does. */
int cffm_expand_candidates(const cffm_shape_t *s, const int32_t *ctx, int32_t C, int32_t field, const int32_t *cand, int32_t N,
                           int64_t first, int32_t rows, int32_t *ids_out, void *stream);
/* cffm_expand_candidates_ex: the same rows for candidates that are TUPLES of nf ids put at nf columns together, from one list for
 * every context or from a list per context.  fields: HOST int32 [nf], distinct columns of [0, F), read before the launch like s (it
 * reaches the kernel by value as a slot map of CFFM_MAX_FIELDS entries: no device copy, no synchronisation).  cand: device int32,
 * id a (a < nf) of candidate n of context c at cand[c * cand_ctx_stride + n * nf + a] (indexed in 64 bits).  cand_ctx_stride == 0:
 * one list [N][nf] for every context; otherwise the elements between the lists of two contexts, >= N * nf - what lies beyond
 * N * nf of a context's block is never read.  For global row g in [first, first + rows), c = g / N, n = g % N:
 * ids_out[g - first][f] = (f == fields[a]) ? cand[c * cand_ctx_stride + n * nf + a] : ctx[c][f].  Writes exactly rows * F int32
 * values.  nf == 1 with stride 0 writes what cffm_expand_candidates writes (that entry point forwards here).
 * CFFM_ERR_BAD_SHAPE, before any launch, for: nf < 1; nf > F; fields == NULL; a field outside [0, F); the same field twice; N < 1;
 * C < 0; first < 0; rows < 0; first + rows > C * N; a negative stride; a non-zero stride below N * nf; a NULL pointer that would
 * be read or written.  C == 0 or rows == 0 returns 0 without a launch. */
int cffm_expand_candidates_ex(const cffm_shape_t *s, const int32_t *ctx, int32_t C, const int32_t *fields, int32_t nf,
                              const int32_t *cand, int64_t cand_ctx_stride, int32_t N, int64_t first, int32_t rows,
                              int32_t *ids_out, void *stream);
/* cffm_topk: for every row c the m = min(k, N - skipped) best candidates in descending order: idx_out[c][j] = candidate position,
 * val_out[c][j] = its score bit for bit (j < m); idx_out[c][j] = -1 and val_out[c][j] = the bits 0x7fc00000 for m <= j < k;
 * count_out[c] = m.  1 <= k <= 1024.  scratch: cffm_topk_scratch_bytes(C, N, k) bytes (< 0 on bad arguments; never smaller for a
 * larger N).  Chunks of 8192 candidates are sorted in LDS by one workgroup each, their k survivors merged level by level. */
int64_t cffm_topk_scratch_bytes(int32_t C, int32_t N, int32_t k);
int cffm_topk(const float *scores, int64_t row_stride, const uint8_t *skip, int64_t skip_stride, int32_t C, int32_t N, int32_t k,
              void *scratch, int32_t *idx_out, float *val_out, int32_t *count_out, void *stream);
/* cffm_rank_of: rank_out[c] = number of non-skipped candidates of row c whose key64 is larger than the one of candidate target[c]
 * (its 0-based rank; the skip flag at the target position itself is ignored); -1 for a target outside [0, N). */
int cffm_rank_of(const float *scores, int64_t row_stride, const uint8_t *skip, int64_t skip_stride, int32_t C, int32_t N,
                 const int32_t *target, int32_t *rank_out, void *stream);

/* ---- candidate sweep with the fixed-field work done once per context (cffm_amd/csrc/sweep.hip) -------
 * Additive entry points: CFFM_ABI_VERSION stays 9, no existing signature, struct or kernel changes.
 * cffm_score_sweep: scores[c * row_stride + n] (indexed in 64 bits) = the raw prediction of context row ctx[c] (int32 [C][F]) with its
 * id at `field` replaced by cand[n] (int32 [N]): the value cffm_predict defines for that id row, to rounding (the sums run in
 * another order), ids clamped the same way (< 0 -> 0, >= M -> M - 1).  Elements n >= N of a row are never written; the ordinary
 * workspace is not touched; scratch: cffm_sweep_scratch_bytes(s, C) bytes (< 0: bad arguments or a shape that is not served; never
 * smaller for a larger C).  A candidate's score does not depend on its position: the same id gives the same bits anywhere in cand,
 * and on every call.  Workgroups take (context, chunk of CFFM_SWEEP_CHUNK candidates) units, so one context with many candidates
 * fills the chip.
 * Served domain (cffm_sweep_ok(s) == 1, host only): both branches on, D = 32, F <= 10 (Pp <= 48), every activation, linear_att 0 and 1,
 * every K whose rows fit the two kernels' LDS next to their tiles (K = 64 at F = 10 does; K <= 2012 at most); D = 64 and F = 11 are not served.
 * CFFM_ERR_UNSUPPORTED where cffm_sweep_ok(s) == 0: after the shape check, before any pointer is read.  CFFM_ERR_BAD_SHAPE, before the
 * first launch or HIP call, for: a NULL pointer that would be read or written; field outside [0, F); N < 1; C < 0; row_stride < N.
 * C == 0 returns 0 without a launch. */
#define CFFM_SWEEP_CHUNK 64
int cffm_sweep_ok(const cffm_shape_t *s);
int64_t cffm_sweep_scratch_bytes(const cffm_shape_t *s, int32_t C);
int cffm_score_sweep(const cffm_shape_t *s, const cffm_tables_t *tab, const float *theta, const int32_t *ctx, int32_t C,
                     int32_t field, const int32_t *cand, int32_t N, float *scores, int64_t row_stride, void *scratch, void *stream);
/* cffm_score_sweep_lists: cffm_score_sweep with a candidate list per context: candidate n of context c is
 * cand[c * cand_ctx_stride + n] (indexed in 64 bits); cand_ctx_stride == 0 is the one shared list, otherwise it is >= N and what lies
 * beyond N of a context's block is never read.  The same two kernels, served domain (cffm_sweep_ok) and scratch
 * (cffm_sweep_scratch_bytes).  A (context, id) pair gives the same bits under a shared list, under its own list, at any position
 * and on every call.  One field only: this and cffm_score_sweep are cffm_score_sweep_tuples (below) with nf = 1.  Refusals: those
 * of cffm_score_sweep, in the same order, plus CFFM_ERR_BAD_SHAPE for a negative stride or a non-zero stride below N. */
int cffm_score_sweep_lists(const cffm_shape_t *s, const cffm_tables_t *tab, const float *theta, const int32_t *ctx, int32_t C,
                           int32_t field, const int32_t *cand, int64_t cand_ctx_stride, int32_t N, float *scores, int64_t row_stride,
                           void *scratch, void *stream);
/* Where the sweep's intermediates lie in the scratch, for the per-stage tests (host only, reads nothing but *s): context c's block
 * starts header_floats + c * block_floats floats into the scratch, and every other member is the offset, in floats from the start
 * of a block, of one tensor the context kernel leaves there (Pp = pairs padded to 16, f = the swept field):
 *   Z [16][16][Pp]  U [2][16][Pp] (dw, y, q)  V [2][16][Pp] (dh, x, q)  Ei [F][K] (row f zero)  s0fix [32]  A [32]
 *   fb [16] (slot f and slots >= F zero)  scal [16] ([0] the inner sum of the pairs without f, [1] R; the rest is never written)
 * What lies between the end of scal and block_floats is never written either.  (header_floats + C * block_floats) * 4 ==
 * cffm_sweep_scratch_bytes(s, C).  Refusals as cffm_sweep_scratch_bytes: CFFM_ERR_BAD_SHAPE for a NULL pointer or a shape the shape
 * check refuses, CFFM_ERR_UNSUPPORTED for a shape that is not served; *out is then untouched.  Additive: the version stays 9. */
typedef struct cffm_sweep_block {
    int64_t header_floats, block_floats;
    int64_t Z, U, V, Ei, s0fix, A, fb, scal;
} cffm_sweep_block_t;
int cffm_sweep_block_layout(const cffm_shape_t *s, cffm_sweep_block_t *out);

/* ---- the shared sweep for candidates that are TUPLES of nf ids (cffm_amd/csrc/sweep.hip) -------------
 * Additive entry points: CFFM_ABI_VERSION stays 9.  cffm_score_sweep_tuples: scores[c * row_stride + n] = the raw prediction of
 * context row ctx[c] with its ids at the nf columns `fields` replaced TOGETHER by candidate n - the value cffm_predict defines for
 * the row cffm_expand_candidates_ex writes, to rounding.  fields: HOST int32 [nf], distinct columns of [0, F) in any order, read
 * before the launch; the library sorts them and carries the column permutation, so fields = {6, 1} with the candidate columns
 * swapped gives the bits of fields = {1, 6}.  cand: device int32, id a of candidate n of context c at
 * cand[c * cand_ctx_stride + n * nf + a] (indexed in 64 bits); cand_ctx_stride == 0: one list [N][nf] for every context, otherwise
 * >= N * nf.  Ids are clamped as cffm_predict clamps them.  A (context, tuple) pair gives the same bits at every position, under a
 * shared list and under its own, and on every call.  One candidate role serves every nf (the field count is compiled in for one field
 * and read at run time for 2 .. CFFM_SWEEP_MAX_NF); cffm_score_sweep and cffm_score_sweep_lists are this function with nf = 1, so
 * nf == 1 here gives their bits.
 * Per context everything that involves no swept field is computed once; per candidate layer 0 costs 4 nf multiply-adds plus 4 per
 * swept-swept pair and output element, the inner branch the pairs with a swept field; above layer 0 nothing changes.
 * Served domain (cffm_sweep_tuples_ok(s, nf) == 1, host only): cffm_sweep_ok(s), 1 <= nf <= min(F, CFFM_SWEEP_MAX_NF), and the
 * candidate kernel's LDS for nf fields within a CU: nf = 2 at every F <= 10 (Pp = 48: 149,184 bytes at K = 32, served up to K = 160
 * at F = 10), nf <= 4 at Pp <= 32; nf = 3 at Pp = 48 is not (164,160 bytes at K = 32).  cffm_sweep_tuples_ok(s, 1) == cffm_sweep_ok(s).
 * scratch: cffm_sweep_tuples_scratch_bytes(s, nf, C) bytes (< 0: bad arguments or not served); linear in C, larger for a larger nf.
 * Refusals, all before the first launch or HIP call, in this order: the shape check; CFFM_ERR_UNSUPPORTED where cffm_sweep_ok(s) == 0;
 * CFFM_ERR_BAD_SHAPE for nf < 1, nf > F, fields == NULL, a field outside [0, F), the same field twice; CFFM_ERR_UNSUPPORTED where
 * cffm_sweep_tuples_ok(s, nf) == 0; CFFM_ERR_BAD_SHAPE for N < 1, C < 0, row_stride < N, a negative stride, a non-zero stride below
 * N * nf; C == 0 returns 0; CFFM_ERR_BAD_SHAPE for a NULL pointer that would be read or written. */
#define CFFM_SWEEP_MAX_NF 4
int cffm_sweep_tuples_ok(const cffm_shape_t *s, int32_t nf);
int64_t cffm_sweep_tuples_scratch_bytes(const cffm_shape_t *s, int32_t nf, int32_t C);
int cffm_score_sweep_tuples(const cffm_shape_t *s, const cffm_tables_t *tab, const float *theta, const int32_t *ctx, int32_t C,
                            const int32_t *fields, int32_t nf, const int32_t *cand, int64_t cand_ctx_stride, int32_t N,
                            float *scores, int64_t row_stride, void *scratch, void *stream);
/* The block of cffm_sweep_block_layout for nf swept fields f_0 < f_1 < ... (sorted, whatever order the caller gave), for the
 * per-stage tests; host only.  Members as there, with
 *   U [nf][2][16][Pp] (a, dw, y, q)  V [nf][2][16][Pp] (a, dh, x, q): field f_a's at U + a * UV_stride, V + a * UV_stride
 *   A [nf][32]: A_a at A + a * A_stride      scal [16]: [0] the inner sum of the pairs without a swept field, [1 + a] R_a
 *   Ei, fb: every swept row / slot zero      Z: the pairs with no swept field
 * U_a, V_a, A_a and R_a run over the fields that are NOT swept below / above f_a.  nf == 1 is the layout of cffm_sweep_block_layout.
 * Refusals as there, for (s, nf) where cffm_sweep_tuples_ok is 0. */
typedef struct cffm_sweep_tuples_block {
    int64_t header_floats, block_floats;
    int64_t Z, U, V, Ei, s0fix, A, fb, scal;
    int64_t UV_stride, A_stride;
} cffm_sweep_tuples_block_t;
int cffm_sweep_tuples_block_layout(const cffm_shape_t *s, int32_t nf, cffm_sweep_tuples_block_t *out);

/* ---- training on ranked lists: backward from a given dL/dout, and two list losses -------------------
 * Additive entry points: CFFM_ABI_VERSION stays 9.  No existing signature, struct, kernel body, default or refusal changes.
 *
 * cffm_backward_dout: the backward half from the CALLER's dL/dout.  The forward was cffm_forward (rows materialised in ws.Ei /
 * ws.Eo / ws.fb; y may have been NULL).  dout: device float [B], used as given: no 1/B, no 1/L, no loss id, and y is not read - so
 * a loss that couples the examples of a batch (the list losses below), or one written in torch on `out`, can be trained.  Leaves
 * what cffm_backward leaves: grad [theta.n], ws.dout (= dout, bit for bit), ws.dt1, ws.dC[l], ws.dEi, ws.dEo, ws.dfb.  Every shape
 * and B takes the stage launches (head, conv layers from the top down, inner branch, slab reduction); the fused backward launches
 * form dL/dout from (out, y, loss) themselves and are never taken.  Any valid s->loss is accepted and not used.
 * Refusals, before any launch: the shape check first (CFFM_ERR_BAD_SHAPE); B <= 0 returns 0 as cffm_backward does;
 * CFFM_ERR_BAD_SHAPE for a NULL theta, dout, ws or grad; CFFM_ERR_UNSUPPORTED for a shape a CU's LDS cannot hold, as cffm_backward. */
int cffm_backward_dout(const cffm_shape_t *s, const float *theta, const float *dout, int32_t B, void *ws, float *grad,
                       void *stream);

/* cffm_list_loss: scores and dout are [G][Lg] contiguous device floats, list g being rows g * Lg .. g * Lg + Lg - 1 in the order
 * cffm_expand_candidates_ex writes them; target[g] (device int32) is the position t of list g's positive.  With m = Lg - 1:
 *   CFFM_LIST_BPR      terms[g] = (1/m) sum_{n != t} softplus(s_n - s_t)
 *                      dout[n] = sigmoid(s_n - s_t) / (G m) for n != t,  dout[t] = -sum_{n != t} dout[n]
 *   CFFM_LIST_SOFTMAX  terms[g] = log sum_n exp(s_n - max) + max - s_t
 *                      dout[n] = (p_n - [n = t]) / G,  p = softmax(s)
 *   loss[0] = (1/G) sum_g terms[g]
 * dout is the gradient of loss[0] with respect to the scores: what cffm_backward_dout takes.  Every exponential has a non-positive
 * argument, so scores of any finite size stay finite.  A NaN score makes its list's term and its whole dout row NaN, and the loss
 * NaN.  A target[g] outside [0, Lg) gives terms[g] = 0 and a zero dout row; nothing is read out of range.  The sums run in a fixed
 * order (one wavefront per list, then two stages in list order): the same bits on every run, whatever scratch held.
 * Writes exactly G * Lg floats of dout, G of terms, one of loss.  scratch: cffm_list_loss_scratch_bytes(G) bytes (-1 for G < 0).
 * CFFM_ERR_BAD_SHAPE, before any launch, for: an unknown kind; G < 0; Lg < 2; G * Lg >= 2^31; a NULL pointer that would be read or
 * written (scores, target, dout, terms, loss, scratch).  G == 0 returns 0 without a launch. */
enum { CFFM_LIST_BPR = 0, CFFM_LIST_SOFTMAX = 1 };
int64_t cffm_list_loss_scratch_bytes(int32_t G);
int cffm_list_loss(int32_t kind, const float *scores, int32_t G, int32_t Lg, const int32_t *target, float *dout, float *terms,
                   float *loss, void *scratch, void *stream);

/* ---- the fused list step: train on ranked lists in the launches of the pointwise step ----------------
 * Additive entry points: CFFM_ABI_VERSION stays 9.  No existing signature, struct, kernel instance, default or refusal changes;
 * cffm_backward_dout keeps the stage launches bit for bit.
 *
 * cffm_list_step_ok: 1 where cffm_train_step_lists is served at B = G * Lg rows, else 0 (also for a shape the shape check refuses or
 * B < 1).  Host only, nothing is launched.  Served: the shapes whose backward runs the fused top, which also places the update's sort
 * keys (both branches on, Pp <= 64 i.e. F <= 11, at least two live conv layers i.e. D >= 8, B <= 256), CFFM_OPT_ADAGRAD, and a loss
 * that is neither CFFM_LOSS_SQUARE_L2 (lamda > 0) nor CFFM_LOSS_LOG (its forward leaves sigmoid(out)). */
int cffm_list_step_ok(const cffm_shape_t *s, int32_t B);
/* cffm_backward_dout_fused: the contract of cffm_backward_dout - after cffm_forward, dout [B] used as given, y not read, leaves what
 * cffm_backward leaves (grad [theta.n], ws.dout = dout bit for bit, ws.dt1, ws.dC[l], ws.dEi, ws.dEo, ws.dfb) - on the launches
 * cffm_backward takes at that (shape, B) where its fused top runs: the fused top with dL/dout read instead of formed (the same kernel
 * body, a compile-time switch), then the one launch for the layers below it or the pair / stage launches, then the slab reduction.
 * Neither ws.scalars nor a loss is written.  Refusals, before any launch: the shape check (CFFM_ERR_BAD_SHAPE); B <= 0 returns 0;
 * CFFM_ERR_BAD_SHAPE for a NULL theta, dout, ws or grad; CFFM_ERR_UNSUPPORTED for a shape a CU's LDS cannot hold and wherever
 * cffm_backward does not take the fused top: B > 256, Pp > 64, a disabled branch, fewer than two live conv layers, CFFM_LOSS_SQUARE_L2. */
int cffm_backward_dout_fused(const cffm_shape_t *s, const float *theta, const float *dout, int32_t B, void *ws, float *grad,
                             void *stream);
/* cffm_train_step_lists: one Adagrad step on G ranked lists of Lg candidates each, B = G * Lg rows, in seven launches at the frappe shape:
 *   1. cffm_expand_candidates_ex(s, ctx, G, fields, nf, cand, cand_stride, Lg, 0, B, ids_out): the id rows, ids_out int32 [B][F]
 *   2. the forward of cffm_train_step on ids_out, without labels: ws.out holds the raw scores.  One launch where the pointwise step
 *      has its single-launch forward (cffm_dp_runs_ok(s, B): D = 32 or 64 with the layer-0 tiles within a CU's LDS, the frappe shape
 *      among them); the stage launches at the other served shapes (F = 11 at D = 32, D = 8, D = 16)
 *   3. cffm_list_loss(kind, ws.out, G, Lg, target, dout, terms, loss, scratch)                         (2 launches)
 *   4. the backward of cffm_train_step from dout (as cffm_backward_dout_fused, which also places the update's sort keys)
 *   5. the fused update of cffm_train_step (slab reduction + dense Adagrad, sorted sparse table update)
 * ctx, fields (HOST), cand, cand_stride as cffm_expand_candidates_ex takes them (N = Lg); target, kind, dout [B], terms [G], loss [1],
 * scratch (cffm_list_loss_scratch_bytes(G) bytes) as cffm_list_loss; the rest as cffm_train_step.  ids_out, dout and terms are the
 * caller's and hold the step's id rows, dL/dout and list terms afterwards; grad holds the dense gradients.
 * Refusals, all with nothing launched, in this order: the shape check; G <= 0 returns 0; CFFM_ERR_BAD_SHAPE for Lg < 2 or an unknown
 * kind; CFFM_ERR_UNSUPPORTED where cffm_list_step_ok(s, G * Lg) == 0; CFFM_ERR_BAD_SHAPE for a NULL pointer; then what
 * cffm_expand_candidates_ex refuses (nf, fields, strides). */
int cffm_train_step_lists(const cffm_shape_t *s, const cffm_tables_t *tab, const cffm_tables_t *tab_acc, float *theta,
                          float *theta_acc, float *grad, const int32_t *ctx, int32_t G, const int32_t *fields, int32_t nf,
                          const int32_t *cand, int64_t cand_stride, int32_t Lg, const int32_t *target, int32_t kind,
                          int32_t *ids_out, float *dout, float *terms, void *ws, float *loss, void *scratch, void *stream);

/* ---- ranked lists drawn on the device, by list id ----------------------------------------------------
 * Additive entry points: CFFM_ABI_VERSION stays 9.  No existing signature, struct, kernel body, default or refusal changes; the
 * table draw (cffm_init_table_rows) keeps its bits.
 *
 * cffm_draw_lists: G lists of m + 1 indices into a set of U distinct tuples.  List g has the id list0 + g and is a function of
 * (seed, id) alone - the same list under every split of an epoch into calls.  at: device int32 [G], the index of each list's
 * positive.  The list holds at[g] and m distinct other indices of [0, U): the length-m prefix of a uniform permutation of the set
 * without at[g] (sparse Fisher-Yates on Philox4x32-10 words, counter (id lo, id hi, word >> 2, 2), key seed), with the positive at a
 * place drawn from word m.  cffm_amd/spec.py draw_lists() is the specification; the match is exact.
 *   lists_out   int32 [G][m + 1] indices, or NULL
 *   tuples_out  int32 [G][m + 1][nf], tuples_out[g][p][a] = cand[lists[g][p]][a] with cand device int32 [U][nf]: the cand operand,
 *               at cand_ctx_stride = (m + 1) * nf, of cffm_expand_candidates_ex and cffm_train_step_lists.  NULL together with cand
 *               for the indices alone (nf is then not used beyond the size check)
 *   target_out  int32 [G], the place of the positive in its list: the target of cffm_list_loss and cffm_rank_of
 * Writes exactly those elements: no scratch, no atomics, the same bits on every call.  A list whose at[g] lies outside [0, U) gets
 * target_out = -1, an index row of -1 and a tuple row of zeros; nothing is read out of range (cffm_list_loss gives such a list a
 * zero term).  One launch.
 * CFFM_ERR_BAD_SHAPE, before any launch, for: U < 2; m < 1; m > U - 1; m > 1023; G < 0; list0 < 0; list0 + G beyond int64;
 * G * (m + 1) * max(nf, 1) >= 2^31; nf < 0; nf == 0 with a non-NULL cand or tuples_out; exactly one of cand / tuples_out NULL; both
 * lists_out and tuples_out NULL; a NULL at or target_out.  G == 0 (with arguments that pass) returns 0 without a launch. */
int cffm_draw_lists(uint64_t seed, int64_t list0, int32_t G, const int32_t *at, int32_t U, int32_t m, const int32_t *cand,
                    int32_t nf, int32_t *lists_out, int32_t *tuples_out, int32_t *target_out, void *stream);

/* ---- weighted ranked lists drawn on the device, by list id --------------------------------------------
 * Additive entry points: CFFM_ABI_VERSION stays 9.  No existing signature, struct, kernel body, default or refusal changes;
 * cffm_draw_lists keeps its bits.
 *
 * cffm_draw_lists_weighted: cffm_draw_lists with the m negatives drawn in proportion to weights - successive sampling without
 * replacement over the set without at[g].  cdf: device uint32 [U], the running sum of the quantised weights as
 * cffm_amd/spec.py weight_cdf() makes it (non-decreasing, total T = cdf[U - 1] <= 2^32 - 1; an index whose entry equals the one
 * before it is never drawn).  T is read on the device; nothing synchronises.  Word i of list id is output word i & 3 of
 * Philox4x32-10 at counter (id lo, id hi, i >> 2, 3), key seed; it gives r = (word * T) >> 32 and the candidate j = #{cdf <= r},
 * clamped to U - 1.  Candidates are taken in word order; one is accepted iff it is not at[g] and was not accepted before, and
 * the negatives are the first m accepted, in that order.  The place of the positive is (word * (m + 1)) >> 32 of output word 0 at
 * counter (id lo, id hi, 0xffffffff, 3).  A list consumes at most 64 * (8 * ceil((m + 1) / 64) + 8) words: one that is still short
 * of m then is INCOMPLETE (heavy skew; rejection sampling, part of the contract).  cffm_amd/spec.py draw_lists_weighted() is the
 * specification; the match is exact.  A cdf that is not non-decreasing gives an unspecified distribution; the search stays inside
 * [0, U) and nothing is read out of range.
 *   lists_out, tuples_out, target_out, cand, nf   as in cffm_draw_lists, NULL rules included
 * An incomplete list, a list whose at[g] lies outside [0, U) and every list when T == 0 get target_out = -1, an index row of -1
 * and a tuple row of zeros.  Writes exactly G * (m + 1) indices, G * (m + 1) * nf tuple words and G targets: one launch, no
 * scratch, no atomics, the same bits on every call.
 * CFFM_ERR_BAD_SHAPE, before any launch, for: U < 1; m < 1; m > U - 1 (so U = 1 is refused); m > 1023; G < 0; list0 < 0; list0 + G
 * beyond int64; G * (m + 1) * max(nf, 1) >= 2^31; nf < 0; nf == 0 with a non-NULL cand or tuples_out; exactly one of cand /
 * tuples_out NULL; both lists_out and tuples_out NULL; a NULL at, target_out or cdf.  G == 0 (with arguments that pass) returns 0
 * without a launch. */
int cffm_draw_lists_weighted(uint64_t seed, int64_t list0, int32_t G, const int32_t *at, int32_t U, int32_t m,
                             const uint32_t *cdf, const int32_t *cand, int32_t nf,
                             int32_t *lists_out, int32_t *tuples_out, int32_t *target_out, void *stream);

/* ---- hard negatives picked from a scored pool, by list id ---------------------------------------------
 * Additive entry points: CFFM_ABI_VERSION stays 9.  No existing signature, struct, kernel body, default or refusal changes;
 * cffm_draw_lists, cffm_draw_lists_weighted and cffm_topk keep their bits.
 *
 * cffm_pick_hard: from the scored pool of each of G lists, the m best-scored negatives around the positive at a drawn place - the
 * select step of dynamic negative sampling.  List g has the id list0 + g.  scores: device fp32, scores[g * row_stride + p] the score
 * of pool position p < Lp (the index is computed in 64 bits; elements at or beyond Lp are never read).  target_pool: device int32
 * [G], t = target_pool[g] the pool position of the list's positive - the target_out of the draw that made the pool.  The negatives
 * are the Lp - 1 positions other than t, ordered by THE ORDER of the candidate ranking above on (score, pool position): score
 * descending, -0 == +0, NaN below -inf, equal scores to the smaller position (the 64-bit key defined there).  The m best are the
 * list's negatives, hardest first.  The positive's place in the list is place = (w * (m + 1)) >> 32, w output word 0 of
 * Philox4x32-10 at counter (id lo, id hi, 0, 4), key seed - the table draw holds 0 and 1 in that last counter word, the list draws
 * 2 and 3 - and the negative of rank r goes to slot r + (r >= place).  With sel[g][slot] the chosen pool position:
 *   lists_out   int32 [G][m + 1], lists_out[g][slot] = pool_lists[g][sel[g][slot]] with pool_lists device int32 [G][Lp]; NULL
 *               together with pool_lists
 *   tuples_out  int32 [G][m + 1][nf], tuples_out[g][slot][a] = pool_tuples[g][sel[g][slot]][a] with pool_tuples device int32
 *               [G][Lp][nf]: the cand operand, at cand_ctx_stride = (m + 1) * nf, of cffm_expand_candidates_ex and
 *               cffm_train_step_lists.  NULL together with pool_tuples (nf is then not used beyond the size check)
 *   target_out  int32 [G] = place, the target of cffm_list_loss and cffm_rank_of
 * A list whose t lies outside [0, Lp) (the draws mark a list without a target and an incomplete list so) gets target_out = -1, an
 * index row of -1 and a tuple row of zeros; nothing of it is read, and nothing is read out of range.  A function of (seed, list id,
 * scores) alone: the place of (seed, id, m), the chosen positions of the scores.  cffm_amd/spec.py pick_hard() is the
 * specification; the match is exact.  Writes exactly G * (m + 1) indices, G * (m + 1) * nf tuple words and G targets: one launch,
 * no scratch, no atomics, the same bits on every call and under every split of the lists into calls.
 * CFFM_ERR_BAD_SHAPE, before any launch, for: Lp < 2; Lp > 1024; m < 1; m > Lp - 1; G < 0; list0 < 0; list0 + G beyond int64;
 * row_stride < Lp; G * Lp * max(nf, 1) >= 2^31; nf < 0; nf == 0 with a non-NULL pool_tuples or tuples_out; exactly one of
 * pool_tuples / tuples_out NULL; exactly one of pool_lists / lists_out NULL; both lists_out and tuples_out NULL; a NULL scores,
 * target_pool or target_out.  G == 0 (with arguments that pass) returns 0 without a launch. */
int cffm_pick_hard(uint64_t seed, int64_t list0, int32_t G, const float *scores, int64_t row_stride, int32_t Lp,
                   const int32_t *target_pool, int32_t m, const int32_t *pool_lists, const int32_t *pool_tuples, int32_t nf,
                   int32_t *lists_out, int32_t *tuples_out, int32_t *target_out, void *stream);

/* ---- logQ-corrected sampled softmax over drawn lists --------------------------------------------------
 * Additive entry points: CFFM_ABI_VERSION stays 9.  No existing signature, struct, kernel body, default or refusal changes;
 * cffm_list_loss and cffm_train_step_lists keep every launch and bit.
 *
 * cffm_list_loss_logq: cffm_list_loss(CFFM_LIST_SOFTMAX) on scores corrected for the proposal the negatives were drawn from.
 * lists: device int32 [G][Lg], lists[g][n] = i_n the index of candidate n among U distinct tuples (lists_out of the draws);
 * corr: device fp32 [U][2], 8-byte aligned, corr[j][0] = log(m q_j) and corr[j][1] = log(1 - q_j) with m = Lg - 1 and q the proposal
 * (cffm_amd/spec.py logq_table() builds it, log m included: the kernel forms no transcendental for the correction).  With t = target[g]:
 *   c_n = corr[i_n][0] - corr[i_t][1]  (n != t),   c_t = 0            z_n = s_n - c_n
 *   terms[g] = log sum_n exp(z_n - max z) + max z - z_t               dout[n] = (softmax(z)_n - [n = t]) / G
 *   loss[0] = (1/G) sum_g terms[g]
 * The positive is in every list with probability 1 and takes no correction; a negative stands for 1 / (m q_n / (1 - q_t)) members of
 * the catalogue without the target: importance sampling of sum_{j != t} exp(s_j) from q_j / (1 - q_t).  An all-zero table gives the
 * bits of cffm_list_loss(CFFM_LIST_SOFTMAX).  Scratch, the two-stage fixed-order loss sum and what is written as cffm_list_loss: the
 * same bits on every run, whatever scratch held.  A target[g] outside [0, Lg) gives a zero row and a zero term and nothing of the list
 * is read; so does any lists[g][n] outside [0, U) in a list with a valid target (tested over the whole list before the first gather:
 * corr is never read out of range).  Repeated indices in a list are allowed.  A non-finite z does what the arithmetic does: the list's
 * term and row become NaN (a -inf correction of a negative among them), as a NaN score does in cffm_list_loss.
 * Refusals, before any launch, in this order: CFFM_ERR_BAD_SHAPE for an unknown kind; CFFM_ERR_UNSUPPORTED for CFFM_LIST_BPR (no
 * agreed correction of the pairwise loss exists); CFFM_ERR_BAD_SHAPE for G < 0, Lg < 2, G * Lg >= 2^31; CFFM_ERR_BAD_SHAPE for U < 1;
 * G == 0 returns 0 without a launch; CFFM_ERR_BAD_SHAPE for a NULL pointer that would be read or written (scores, target, lists, corr,
 * dout, terms, loss, scratch) and for a corr that is not 8-byte aligned. */
int cffm_list_loss_logq(int32_t kind, const float *scores, int32_t G, int32_t Lg, const int32_t *target,
                        const int32_t *lists, const float *corr, int32_t U,
                        float *dout, float *terms, float *loss, void *scratch, void *stream);
/* cffm_train_step_lists_logq: cffm_train_step_lists with its step 3 replaced by cffm_list_loss_logq(kind, ws.out, G, Lg, target, lists,
 * corr, U, dout, terms, loss, scratch) - the same launches (seven at the frappe shape), the same served domain (cffm_list_step_ok).
 * Every argument of cffm_train_step_lists in its order up to scratch, then lists, corr, U as above.  Refusals, all with nothing
 * launched, in the order of cffm_train_step_lists with two more: CFFM_ERR_UNSUPPORTED for CFFM_LIST_BPR right after the kind check,
 * and CFFM_ERR_BAD_SHAPE for U < 1, a NULL lists, a NULL corr or a corr that is not 8-byte aligned right after the NULL checks. */
int cffm_train_step_lists_logq(const cffm_shape_t *s, const cffm_tables_t *tab, const cffm_tables_t *tab_acc, float *theta,
                               float *theta_acc, float *grad, const int32_t *ctx, int32_t G, const int32_t *fields, int32_t nf,
                               const int32_t *cand, int64_t cand_stride, int32_t Lg, const int32_t *target, int32_t kind,
                               int32_t *ids_out, float *dout, float *terms, void *ws, float *loss, void *scratch,
                               const int32_t *lists, const float *corr, int32_t U, void *stream);

/* ---- the skip mask of a ranking call from a sparse "seen" relation (cffm_amd/csrc/seen.hip) ---------------
 * Additive entry point: CFFM_ABI_VERSION stays 9.  No existing signature, struct, kernel body, default or refusal changes; the mask
 * is consumed by the unchanged cffm_topk and cffm_rank_of as their `skip`.
 *
 * The relation is a CSR on the device: off int32 [R + 1] row offsets, pos int32 [nnz] candidate POSITIONS of the call, and per
 * context the CSR row row[c] (int32 [C]).  cffm_seen_mask: for every c < C and n < N, mask_out[c * mask_stride + n] = 1 where
 *   skip_in != NULL and skip_in[c * skip_in_stride + n] != 0, or
 *   n == pos[j] for a j in [lo, hi), lo = min(max(off[r], 0), nnz), hi = min(max(off[r + 1], 0), nnz), r = row[c] in [0, R)
 * and 0 otherwise.  Exactly C * N bytes are written, each once; the bytes [N, mask_stride) of a row are never touched, and what
 * mask_out held before does not matter.  pos within a row may come in any order and may repeat; an entry outside [0, N) is ignored.
 * A row[c] outside [0, R), off[r + 1] < off[r] and offsets outside [0, nnz] (clamped as above) give an empty or shortened seen set and
 * never an out-of-range read: whatever the device arrays hold, the kernel reads only inside off[0..R], pos[0..nnz), row[0..C) and
 * the first N bytes of the rows of skip_in.  skip_in and mask_out must not overlap anywhere (the kernel takes both as restrict-qualified;
 * only the identical pointer is detected and refused, any other overlap is undefined).  No atomics; the same bytes on every run.  cffm_amd/spec.py seen_mask() is the numpy twin.
 * CFFM_ERR_BAD_SHAPE, before any launch or HIP call, whatever C is, for: a NULL off, row or mask_out, a NULL pos with nnz != 0
 * (skip_in may be NULL); N < 1, C < 0, R < 0 or nnz < 0; mask_stride < N; skip_in_stride < N with skip_in != NULL;
 * skip_in == mask_out.  C == 0 (with arguments that pass) returns 0 without a launch. */
int cffm_seen_mask(const int32_t *off, const int32_t *pos, int32_t R, int64_t nnz, const int32_t *row, const uint8_t *skip_in,
                   int64_t skip_in_stride, int32_t C, int32_t N, uint8_t *mask_out, int64_t mask_stride, void *stream);

/* ---- peak probes (bench.py prices the kernels against the data-sheet peaks AND these measured ones) ------------- */
/* float4 streaming copy src -> dst (bytes % 16 == 0): 2*bytes of HBM traffic per launch */
int cffm_probe_copy(const void *src, void *dst, int64_t bytes, void *stream);
/* read-only stream of `bytes` (the HBM READ roofline a gather is priced against); sink: >= 2048 floats, practically never written */
int cffm_probe_read(const void *src, void *sink, int64_t bytes, void *stream);
/* dependency-free fp32 MFMA loop over the whole chip; *flops receives the flop count of the launch */
int cffm_probe_mfma(float *out, int32_t iters, int64_t *flops, void *stream);
/* the same on the bf16 pipe (v_mfma_f32_16x16x32_bf16): the denominator of the bf16x3 conv loops */
int cffm_probe_mfma_bf16(float *out, int32_t iters, int64_t *flops, void *stream);
/* exactly ONE v_mfma_f32_16x16x32_bf16 per problem, D = A B + C on the caller's operands (one wavefront each): n problems of
 * A [16][32] and B [32][16] as bf16 bit patterns (A 16-byte aligned), C and D [16][16] fp32, all row-major on the device.
 * What the accumulate of the bf16x3 conv loops rounds to is read from this (oracle/mfma_model.py).  n == 0 returns 0 without a
 * launch; CFFM_ERR_BAD_SHAPE for n < 0 or a NULL / misaligned pointer with n > 0. */
int cffm_probe_mfma_bf16_once(const uint16_t *A, const uint16_t *B, const float *C, float *D, int32_t n, void *stream);

/* The same step for the other optimizers of CFFM.py:517-529 (s->optimizer): state1 = Momentum accumulators / Adam m,
 * state2 = Adam v (NULL otherwise), step = 1-based Adam time step.  Adagrad routes to cffm_train_step(state1). */
int cffm_train_step_opt(const cffm_shape_t *s, const cffm_tables_t *tab, const cffm_tables_t *tab_state1,
                        const cffm_tables_t *tab_state2, float *theta, float *theta_state1, float *theta_state2,
                        float *grad, const int32_t *ids, const float *y, int32_t B, void *ws, float *loss, int64_t step,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CFFM_HIP_H */

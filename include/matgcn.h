/*
 * matgcn.h - C ABI of the MI355X-native Multi-ATGCN forward hot path (libmatgcn.so).
 *
 * This is the drop-in boundary for ONE path of SonghuaHu-UMD/MultiSTGraph: MultiATGCN.forward()
 * (reference libcity/model/traffic_flow_prediction/MultiATGCN.py:363-420) and the pieces it is
 * made of.  The reference has no FFI of its own (it is 100 % Python/torch), so each entry point
 * names the reference symbol it replaces; the Python class that binds them through ctypes is
 * multistgraph_amd/model.py (the binding a maintainer would add is shown in INTEGRATION.md).
 *
 * Conventions
 *   - every function returns MATGCN_OK (0) or a negative matgcn_status; no exceptions, no device
 *     allocation, no implicit synchronisation: work is enqueued on the caller's hipStream_t
 *     (passed as void*) - internally forked onto library-owned streams that join back before the
 *     call's last kernel - and the caller owns every buffer including `prepared` and `workspace`.
 *   - every pointer in matgcn_params / X / out / prepared / workspace is a DEVICE pointer to
 *     contiguous row-major fp32, 16-byte aligned (torch allocations are 256-byte aligned).
 *   - matgcn_dims is a plain host struct, read at call time.
 *   - shapes use the reference's names: B batch, T = input_window (24), N nodes, H = rnn_units,
 *     F = feature dim of batch['X'], K = stacked supports including the identity.
 *   - an entry point that fails between forking onto the library streams and joining them joins them into the caller's
 *     stream before it returns its error code: the caller's buffers are quiet once its own stream is.
 *
 * ABI 10 (round 3) over ABI 9: matgcn_metric_sums / matgcn_metric_table (the evaluator's table and the group-std
 * re-transform on the device), matgcn_series_violations (range contract of the series entry points: rows are clamped
 * and counted, never read out of bounds), matgcn_set_mix_precision(2) (bf16 operands for the node-wise contractions),
 * a batch-split forward switch, matgcn_set_lazy_prepare / matgcn_prepare_join; matgcn_workspace_bytes also covers two
 * half-batch plans and the bf16 copies of the weight streams.  No signature of ABI 9 changed.
 * ABI 12 over ABI 11: the batch-split forward switch and the lab schedule matgcn_set_wavefront(2) are removed (any
 * non-zero value now selects the wavefront); matgcn_workspace_bytes no longer counts two half-batch plans.
 * Still ABI 12: matgcn_set_mix_precision(3) (three bf16 pieces per operand of the graph mixes) is one more value of an
 * existing argument - no symbol, signature or struct changed, and every value ABI 12 defined keeps its meaning and bits.
 * Still ABI 12: matgcn_set_deterministic is one more symbol - no existing symbol, signature or struct changed, and with
 * the setting at its default (0) matgcn_train_bytes and matgcn_backward are what ABI 12 defined.
 * Still ABI 12: matgcn_set_train_bf16x3 is one more symbol, on the same terms - with it at its default (0) every entry
 * point launches the kernels ABI 12 defined, with their arguments and bits, and both *_bytes() give its numbers;
 * matgcn_set_train_precision keeps every value's meaning (3 included: it means 0).
 * Still ABI 12: device-side dropout adds five names - the struct matgcn_dropout and the functions matgcn_dropout_mask,
 * matgcn_forward_train_seeded, matgcn_backward_seeded, matgcn_forward_mc - and nothing else changes: no existing symbol,
 * signature or struct changed, both *_bytes() give their numbers, and a caller that hands matgcn_forward_train /
 * matgcn_backward a mask tensor (or NULL) launches the kernels ABI 12 defined, with their arguments and bits.
 * Still ABI 12: quantiles and scores of a Monte-Carlo-dropout ensemble add three functions - matgcn_mc_quantiles,
 * matgcn_mc_scores_bytes, matgcn_mc_scores - and two constants; no existing symbol, signature, struct or value changed, and
 * matgcn_forward_mc launches the kernel it launched, with its arguments and bits.
 * Still ABI 12: new names only - the device-side optimizer step adds the structs matgcn_opt_tensor and matgcn_adam and the
 * functions matgcn_grad_norm_bytes, matgcn_grad_norm, matgcn_adam_step; no existing symbol, signature, struct or value
 * changed, and no existing entry point launches anything else than it did.
 * Still ABI 12: new names only - the per-node evaluation tables add the functions matgcn_metric_sums_nodes_bytes,
 * matgcn_metric_sums_nodes, matgcn_metric_table_rows, matgcn_mc_quantiles_scaled, matgcn_mc_scores_nodes_bytes and
 * matgcn_mc_scores_nodes; no existing symbol, signature, struct or value changed, and no existing entry point launches
 * anything else than it did, with other arguments or other bits.
 * Still ABI 12: new names only - the training objectives add the enum MATGCN_LOSS_*, the struct matgcn_loss_desc and the
 * functions matgcn_loss_bytes, matgcn_loss and matgcn_loss_grad; matgcn_masked_mae / matgcn_masked_mae_grad are what they
 * were, and no existing symbol, signature, struct or value changed.
 * Still ABI 12: new names only - conformal calibration of the Monte-Carlo-dropout band adds the functions
 * matgcn_mc_conformity, matgcn_conformal_quantile and matgcn_conformal_coverage; no existing symbol, signature, struct or
 * value changed, and no existing entry point launches anything else than it did.
 * Still ABI 12: new names only - the region-level training loss adds the functions matgcn_region_loss_bytes,
 * matgcn_region_loss and matgcn_region_loss_grad; no existing symbol, signature, struct or value changed.
 * Still ABI 12: new names only - training on the CRPS of the Monte-Carlo-dropout ensemble adds the functions
 * matgcn_train_mc_bytes, matgcn_forward_train_mc, matgcn_backward_mc, matgcn_crps_loss_bytes, matgcn_crps_loss and
 * matgcn_crps_loss_grad; no existing symbol, signature, struct or value changed, both *_bytes() of the training step give
 * their numbers, and no existing entry point launches anything else than it did.
 */
#ifndef MATGCN_H
#define MATGCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MATGCN_ABI_VERSION 12

typedef enum matgcn_status {
  MATGCN_OK = 0,
  MATGCN_ERR_NULL = -1,        /* a required pointer is NULL */
  MATGCN_ERR_BAD_ARG = -2,     /* inconsistent / out-of-range dims */
  MATGCN_ERR_UNSUPPORTED = -3, /* valid in the reference, not built yet */
  MATGCN_ERR_SMALL_BUFFER = -4,/* prepared / workspace smaller than *_bytes() reports */
  MATGCN_ERR_LAUNCH = -5       /* hipGetLastError() != hipSuccess after a launch */
} matgcn_status;

/* adaptive adjacency mode = config['adpadj'] (MultiATGCN.py:80-85) */
enum { MATGCN_ADP_NONE = 0, MATGCN_ADP_UNI = 1, MATGCN_ADP_BI = 2 };

#define MATGCN_MAX_LAYERS 4
#define MATGCN_MAX_HEADS 8
#define MATGCN_MAX_EXT 16
#define MATGCN_MAX_XSTEPS 256 /* x_steps accepted by matgcn_forward_series */

typedef struct matgcn_dims {
  int32_t batch;        /* B */
  int32_t nodes;        /* N */
  int32_t in_steps;     /* T = input_window; the reference hard-codes 24-step heads (:373-393) */
  int32_t x_steps;      /* steps of batch['X'] = len_closeness+len_period+len_trend (96) */
  int32_t x_feat;       /* F */
  int32_t out_channels; /* output_window * output_dim = Conv2d out channels (:340) */
  int32_t out_dim;      /* output_dim = end_dim - start_dim (:320) */
  int32_t start_dim;    /* first flow channel of X (:365) */
  int32_t hidden;       /* H = rnn_units; this build: 64 */
  int32_t layers;       /* num_layers */
  int32_t feat_in;      /* feature_final = out_dim + ext channels fed to layer 0 (:321) */
  int32_t embed_dim;    /* d = node_emb columns */
  int32_t adj_rank;     /* r = node_vec1 columns (unidirection) */
  int32_t adp_mode;     /* MATGCN_ADP_* */
  int32_t n_static;     /* first-order static supports used by the stack (0..3), (:87-93) */
  int32_t cheb_k;       /* cheb_order (>= 1; 1 = one weight broadcast over [I, S_1, S_2, ..], :65-70,94-108) */
  int32_t scale_by_g;   /* 1 iff adjtype == 'multi': stack *= softmax(weights_g) (:102-103) */
  int32_t n_heads;      /* temporal heads fused (2 if output_window < 6 else 4, :371-393) */
  int32_t n_ts;         /* len(weight_tsg) = len_ts (:328-332) */
  int32_t diag_static_mask; /* bit s set: static support s is a diagonal matrix (host-checked, e.g. the
                           * similarity Laplacian -I without static features, :244-250).  Such supports are
                           * folded into the identity slot of the node-adaptive weights and never mixed. */
  int32_t gcn_off;      /* 1: ablation without graph convolution - encoder.agru_cells are dense GRU cells, no
                         * residual cells, no blend (:177-192,205-208); their nn.Linear weights are passed in
                         * matgcn_params.res_gate / res_update, the AGCN / support fields are ignored */
  int32_t fnn_off;      /* 1: ablation of the temporal head - end_conv sees the last step only (:342-344,412) */
  int32_t head_begin[MATGCN_MAX_HEADS]; /* first X step of head h (trend head never advances) */
  int32_t ext_src[MATGCN_MAX_EXT];      /* X channel copied into encoder channel out_dim+j */
} matgcn_dims;

typedef struct matgcn_agcn_params { /* one AGCN (MultiATGCN.py:71-73) */
  const float* weights_g;    /* (K,1,1) */
  const float* weights_pool; /* (d, K, I, O) */
  const float* bias_pool;    /* (d, O) */
} matgcn_agcn_params;

typedef struct matgcn_linear_params { /* one nn.Linear of the residual GRUCell (:139-140) */
  const float* weight; /* (O, I) */
  const float* bias;   /* (O) */
} matgcn_linear_params;

typedef struct matgcn_params { /* device pointers, names = the reference state_dict keys */
  const float* node_emb;        /* (N, d) */
  const float* node_vec1;       /* (N, r)  or NULL */
  const float* node_vec2;       /* (r, N)  or NULL */
  const float* static_supports; /* (n_static, N, N): model.supports[s][1] (:264-283) or NULL */
  const float* weight_tsg;      /* (n_ts) */
  const float* weight_ts[MATGCN_MAX_HEADS]; /* each (1,24,N,out_dim) */
  const float* weights_gru;     /* encoder.weights_gru (L, T) */
  matgcn_agcn_params gate[MATGCN_MAX_LAYERS];     /* encoder.agru_cells.l.gate   (O = 2H) */
  matgcn_agcn_params update[MATGCN_MAX_LAYERS];   /* encoder.agru_cells.l.update (O = H)  */
  matgcn_linear_params res_gate[MATGCN_MAX_LAYERS];   /* encoder.res_cells.l.gate   */
  matgcn_linear_params res_update[MATGCN_MAX_LAYERS]; /* encoder.res_cells.l.update */
  const float* end_conv_weight; /* (out_channels, T, 1, H); (out_channels, 1, 1, H) with fnn_off */
  const float* end_conv_bias;   /* (out_channels) */
} matgcn_params;

/* ---- introspection ------------------------------------------------------------------------ */
int matgcn_abi_version(void);
const char* matgcn_error_string(int status);

/* Bytes of the two caller-owned device buffers for `dims`.  matgcn_workspace_bytes depends on two library settings: while
 * matgcn_set_mix_precision(2) or matgcn_set_train_precision(2) is in force it also counts the bf16 copies of the recurrent
 * weight streams (half the bytes of the fp32 streams, behind everything else); a mode-2 forward on a workspace sized
 * without them returns MATGCN_ERR_SMALL_BUFFER (ask again and re-allocate).  While matgcn_set_mix_precision(3) is in force
 * it counts the three bf16 planes of the support stack instead (6 bytes per element of the [Np up to 32][Ks*Np up to 64]
 * stack), under the same contract; likewise while matgcn_set_train_bf16x3 is the effective training mode (see there).  The
 * fp32 paths never pay for either. */
int matgcn_prepared_bytes(const matgcn_dims* dims, size_t* bytes);
int matgcn_workspace_bytes(const matgcn_dims* dims, size_t* bytes);

/* Where the transposed support stack lives inside `prepared` (for tests / debugging):
 * out[0] = float offset, out[1] = leading dimension, out[2] = padded node count Np,
 * out[3] = number of DENSE non-identity slots Ks (diagonal supports are folded away, in stack order
 * otherwise).  Element S_k[n][m] of dense slot k is at prepared[out[0] + m*out[1] + k*Np + n]. */
int matgcn_supports_layout(const matgcn_dims* dims, int64_t out[4]);

/* Where the RECURRENT rows of a node-adaptive weight stream live inside `prepared` (for tests: what matgcn_prepare
 * really wrote, including diagonal supports folded into the identity slot and softmax(weights_g)).
 * part 0 = agru_cells[layer].gate (O = 128), 1 = .update (O = 64).  out[0] = float offset of node 0, out[1] = floats
 * between nodes, out[2] = k-groups of 16 rows (= 4 * (1 + Ks)), out[3] = column tiles O/16.  Row kk = 64*slot + c is
 * hidden channel c of node-GEMM slot `slot` (0 = identity, then the dense slots); W_n[kk][o] is at
 *   out[0] + n*out[1] + (((kk/16)*out[3] + o/16)*64 + (o%16) + 16*((kk%16)/4))*4 + kk%4   (v_mfma_f32_16x16x4 B order). */
int matgcn_weights_layout(const matgcn_dims* dims, int layer, int part, int64_t out[4]);

/* ---- parameter-only work, once per parameter update ----------------------------------------
 * Replaces what AGCN.forward rebuilds on every call (MultiATGCN.py:78-105): the adaptive adjacency
 * softmax(relu(E1 E2)) / softmax(relu(E E^T)), the Chebyshev support stack, the node-adaptive
 * weights einsum('nd,dkio->nkio') and bias, with softmax(weights_g) folded into the weights; plus
 * MFMA-fragment-ordered copies of the residual-GRU and Conv2d-head weights. */
int matgcn_prepare(const matgcn_dims* dims, const matgcn_params* params, void* prepared,
                   size_t prepared_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the path ------------------------------------------------------------------------------
 * MultiATGCN.forward / predict (MultiATGCN.py:363-420, eval mode):
 * X (B, x_steps, N, F) -> out (B, output_window, N, output_dim).
 * h0: initial state of the encoder, (L, B, N, H) device, or NULL for the zero state of init_hidden (:214-218, :405).
 * With static features the reference starts every layer and sample from static_initial_gru(static @ v) (:406-409):
 * that (N, H) embedding is host-side torch (a PCA and one nn.Linear), expanded to (L, B, N, H) by the caller. */
int matgcn_forward(const matgcn_dims* dims, const matgcn_params* params, const void* prepared,
                   const float* X, const float* h0, float* out, void* workspace, size_t workspace_bytes,
                   void* stream);

/* The same forward fed from the raw series instead of materialised windows (replaces the window build of
 * MTHDataset._generate_input_data, libcity/data/dataset/dataset_subclass/mth_dataset.py:110-160, and the
 * per-batch host copy of data/utils.py:68-72 + batch.py:43-57): series (series_steps, N, F) resident on the
 * device, label_start (B) device int32 - the first target step of each sample -, rel_steps (x_steps) HOST
 * int32 - offset of every window row relative to its label start (multistgraph_amd/windows.py).
 * Row s of sample b is series[label_start[b] + rel_steps[s]]; the caller guarantees they are in range
 * (multistgraph_amd/windows.py::check_label_starts validates a table on the host where it is built).  The kernels
 * never read outside the series all the same: an out-of-range row is clamped to the first / last row and counted,
 * see matgcn_series_violations. */
int matgcn_forward_series(const matgcn_dims* dims, const matgcn_params* params, const void* prepared,
                          const float* series, int64_t series_steps, const int32_t* label_start,
                          const int32_t* rel_steps, const float* h0, float* out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The batch as B label starts into the device-resident raw series instead of materialised windows: what
 * matgcn_forward_series takes as separate arguments, as one descriptor for the training entry points. */
typedef struct matgcn_series {
  const float* series;        /* (series_steps, N, F) device */
  int64_t series_steps;
  const int32_t* label_start; /* (B) device: first target step of every sample */
  const int32_t* rel_steps;   /* (x_steps) HOST: offset of every window row relative to its label start */
} matgcn_series;

/* Diagnostic for the series entry points (matgcn_forward_series, the matgcn_series source of the training calls,
 * matgcn_masked_mae{,_grad} with label_start): number of row accesses on the CURRENT device, since the last reset,
 * whose index label_start[b] + offset fell outside the series and was clamped.  0 = the range contract held.
 * Synchronises the device (a debugging / validation call, not part of a step); reset != 0 clears the counter. */
int matgcn_series_violations(int64_t* count, int reset);

/* ---- the pieces (same kernels, exposed for parity tests against the reference's modules) ----
 * temporal-head fusion + channel concat (MultiATGCN.py:365-402): X -> x0 (B, T, N, feat_in) */
int matgcn_fuse_heads(const matgcn_dims* dims, const matgcn_params* params, const float* X,
                      float* x0, void* workspace, size_t workspace_bytes, void* stream);

/* AGCN.forward of agru_cells[layer].gate on cat(x, h) (MultiATGCN.py:76-109):
 * x (B,N,C_l), h (B,N,H) -> y (B,N,2H), no activation. */
int matgcn_agcn_gate_fwd(const matgcn_dims* dims, const matgcn_params* params,
                         const void* prepared, int layer, const float* x, const float* h,
                         float* y, void* workspace, size_t workspace_bytes, void* stream);

/* ATGRUCell.forward of agru_cells[layer] (MultiATGCN.py:120-128): x, h -> h_out (B,N,H) */
int matgcn_atgru_cell_fwd(const matgcn_dims* dims, const matgcn_params* params,
                          const void* prepared, int layer, const float* x, const float* h,
                          float* h_out, void* workspace, size_t workspace_bytes, void* stream);

/* GRUCell.forward of res_cells[layer] (MultiATGCN.py:142-150): x, h -> h_out (B,N,H) */
int matgcn_res_cell_fwd(const matgcn_dims* dims, const matgcn_params* params,
                        const void* prepared, int layer, const float* x, const float* h,
                        float* h_out, void* workspace, size_t workspace_bytes, void* stream);

/* ATGRUEncoder.forward (MultiATGCN.py:194-212): x0 (B,T,N,feat_in), h0 (L,B,N,H) or NULL (zeros)
 * -> seq (B,T,N,H) of the last layer and finals (L,B,N,H); either output may be NULL. */
int matgcn_encoder_fwd(const matgcn_dims* dims, const matgcn_params* params, const void* prepared,
                       const float* x0, const float* h0, float* seq, float* finals,
                       void* workspace, size_t workspace_bytes, void* stream);

/* end_conv + reshape/permute (MultiATGCN.py:416-418, eval): seq (B,T,N,H) -> out */
int matgcn_output_head(const matgcn_dims* dims, const matgcn_params* params, const void* prepared,
                       const float* seq, float* out, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- loss / metric epilogue ---------------------------------------------------------------------
 * De-scale, mask and reduce on the device (MultiATGCN.calculate_loss, MultiATGCN.py:422-427, with
 * loss.masked_mae_torch, libcity/model/loss.py:17-29; TrafficStateEvaluator "single" mode MAE@k,
 * libcity/evaluator/traffic_state_evaluator.py:87-104).  For an affine scaler x -> x*std + mean:
 *   l = y*std + mean, p = pred*std + mean;  l := 0 where |l| < min_s;
 *   mask = (l != null_val)   [null_val NaN: mask = !isnan(l)]
 *   result[0]     = sum(|p-l|*mask) / sum(mask)              (the masked-MAE loss over all horizons)
 *   result[1 + k] = the same restricted to horizon k          (MAE@k+1)
 * pred (B, out, N, od) contiguous; y (B, y_steps >= out, N, y_feat), channels y_start .. y_start+od-1.
 * label_start != NULL (device, B int32): `y` is the raw series (y_steps, N, y_feat) instead and the label rows of
 * sample b are y[label_start[b] + o], o < out - the targets MTHDataset._generate_input_data materialises
 * (mth_dataset.py:110-160) are gathered here, on the device.
 * The label contract - of every entry point that takes (y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat,
 * y_start): the four counts >= 1, 0 <= y_start and y_start + out_dim <= y_feat, and one of two rules for y_steps -
 *   strict rule  y_steps >= out_steps, windows or series: matgcn_masked_mae{,_grad}, matgcn_loss{,_grad},
 *                matgcn_metric_sums{,_nodes}, matgcn_region_loss{,_grad};
 *   series rule  y_steps >= 1 and y_feat >= 1, and y_steps >= out_steps for windows only: matgcn_mc_scores{,_nodes},
 *                matgcn_mc_conformity, matgcn_group_label_sums
 * - else MATGCN_ERR_BAD_ARG, before any launch.
 * partials: caller-owned device scratch of 2*B*out + 1 floats (the last one keeps sum(mask) for the gradient);
 * result: device, 1+out floats.  Two launches, fixed summation order (no atomics): results are run-to-run identical. */
int matgcn_masked_mae(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                      int out_dim, int y_steps, int y_feat, int y_start, float mean, float std, float null_val,
                      float min_s, float* partials, float* result, void* stream);

/* Gradient of result[0] (the calculate_loss value) w.r.t. pred, for the training step: d_pred (B, out, N, od) =
 * upstream[0] * std * sign(p - l) * mask / sum(mask), with `partials` as left by the matching matgcn_masked_mae call
 * and `upstream` the device scalar autograd hands down (d loss / d loss = 1 for a plain loss.backward()). */
int matgcn_masked_mae_grad(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps,
                           int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean, float std,
                           float null_val, float min_s, const float* partials, const float* upstream, float* d_pred,
                           void* stream);

/* ---- the executor's training objectives, value and gradient (matgcn_loss.hip) ---------------------------------------
 * TrafficStateExecutor._build_train_loss (libcity/executor/traffic_state_executor.py:200-250) offers eleven
 * differentiable objectives; they are seven kinds here (the `masked_*` names are the first four with null_val = 0):
 *   MAE, MSE, RMSE, MAPE   loss.masked_{mae,mse,rmse,mape}_torch (libcity/model/loss.py:17-90) - the MASKED kinds:
 *                          l := 0 where |l| < min_s;  m = (l != null_val) [null_val NaN: m = !isnan(l)];
 *                          value = sum(t*m) / sum(m);  a term that is NaN after masking adds 0 and gets gradient 0, an
 *                          infinite one stays infinite (MAPE on an unmasked zero label), nothing kept gives 0.
 *   LOGCOSH, HUBER, QUANTILE   loss.log_cosh_loss, huber_loss, quantile_loss (loss.py:32-51): the plain mean over all
 *                          B*out*N*od elements - no min_s, no mask (both fields ignored); a NaN label makes the value NaN.
 * With l = y*std + mean, p = pred*std + mean (two fp32 roundings each, like the reference's tensors), d = p - l (fp32):
 *   kind       term t                                               g = dt/dp
 *   MAE        |d|                                                  sign(d), 0 at 0
 *   MSE        d^2                                                  2 d
 *   RMSE       as MSE; the value is sqrt(mse)                       2 d / (2 rmse); ALL gradients 0 when rmse == 0
 *                                                                   (torch divides 0 by 0 there and gives NaN)
 *   MAPE       |d / l|                                              sign(d) / |l|
 *   LOGCOSH    |d| + log1p(exp(-2|d|)) - ln 2                       tanh(d)
 *   HUBER      0.5 d^2 if |d| <= delta else delta |d| - 0.5 delta^2  d if |d| <= delta else delta sign(d)
 *   QUANTILE   delta (l - p) if l >= p else (1 - delta)(p - l)      -delta if l >= p else 1 - delta
 * LOGCOSH is the one deliberate departure from the reference's float32 bits: its log(cosh(d)) overflows to inf in float32
 * once |d| passes about 89, which de-scaled visit counts do routinely; the form above is the same function and stays finite.
 * Terms, sums, quotient and square root are fp64 and every result is rounded to float32 once:
 *   result[0] = the objective over all horizons (what the executor trains on), result[1 + k] = the same over horizon k.
 * Geometry arguments as the masked-MAE pair above (label_start != NULL: y is the raw series; out_steps in 1 .. 64).
 * scratch: caller-owned device memory of the size the bytes query below reports - two doubles (term sum, count) per
 * (b, horizon) slab from stage 1, then the count over all horizons and the fp64 mse, which stage 2 keeps for the gradient;
 * every word read is written first by the same call.  Two launches, fixed summation order, no atomics: two calls give the
 * same bits.  The gradient call - d_pred (B, out, N, od) = upstream[0] * std * g * m / count, formed in fp64 and rounded
 * once - takes the scratch its value call left (the unmasked kinds read nothing from it: their count is the element
 * count) and the same geometry and descriptor; `upstream` is the device scalar autograd hands down.
 * Every argument is checked on the host before any launch: a kind outside the enum, a delta that is not finite, a
 * QUANTILE delta outside (0, 1) or a HUBER delta <= 0 is MATGCN_ERR_BAD_ARG (delta is ignored by the other kinds only in
 * the arithmetic), a short scratch MATGCN_ERR_SMALL_BUFFER, index spaces of 2^31 or more MATGCN_ERR_UNSUPPORTED.  Nothing
 * is allocated; only the caller's stream is used. */
enum { MATGCN_LOSS_MAE = 0, MATGCN_LOSS_MSE, MATGCN_LOSS_RMSE, MATGCN_LOSS_MAPE,
       MATGCN_LOSS_LOGCOSH, MATGCN_LOSS_HUBER, MATGCN_LOSS_QUANTILE };
typedef struct matgcn_loss_desc {
  int32_t kind;       /* MATGCN_LOSS_* */
  float mean, std;    /* the scaler's affine x*std + mean */
  float null_val;     /* MASKED kinds: the label value left out (NaN: NaN labels) */
  float min_s;        /* MASKED kinds: |l| < min_s -> 0 */
  float delta;        /* HUBER: the knee (> 0); QUANTILE: the level (0 < delta < 1); finite for every kind */
} matgcn_loss_desc;
int matgcn_loss_bytes(int batch, int out_steps, size_t* bytes);
int matgcn_loss(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc, void* scratch,
                size_t scratch_bytes, float* result /* 1 + out_steps */, void* stream);
int matgcn_loss_grad(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                     int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc, const void* scratch,
                     size_t scratch_bytes, const float* upstream, float* d_pred, void* stream);

/* ---- the evaluator's metric table on the device ------------------------------------
 * TrafficStateEvaluator.collect (libcity/evaluator/traffic_state_evaluator.py:34-121: ten metrics per horizon, modes
 * "single" and "average") and the group-std re-transform table of TrafficStateExecutor.evaluate
 * (libcity/executor/traffic_state_executor.py:293-322) without copying predictions to the host: one pass over
 * prediction and label reduces, per horizon, the MATGCN_METRIC_SUMS sums every metric is a ratio of (fp64), and
 * matgcn_metric_table turns (accumulated) sums into the table.
 *   l = y, p = pred;  first affine x*std + mean (scalar, or one pair per node: per_node) - the scaler's
 *   inverse_transform (:268-273);  second affine per node - prediction_t = prediction * All_std + All_m (:307-308);
 *   each affine two fp32 roundings, as the reference's tensors (a fused one moves |d/l| of a label near 0);
 *   p := clamp_min where p < clamp_min (:312);  elements with l <= truth_min are left out (:316-317);
 *   l := 0 where |l| < min_s (loss.py:18, 53, 71; min_s < 0: off - the *_np functions of the re-transform do not).
 * sums per horizon: 0 elements, 1 non-NaN labels, 2 sum|p-l|, 3 sum (p-l)^2, 4 sum |(p-l)/l| (NaN terms -> 0, as
 * loss.py does) over those, 5 labels != 0, 6-8 the same three over those, 9 sum l, 10 sum l^2, 11 sum p, 12 sum p^2,
 * 13 sum (l-p).  Geometry arguments as matgcn_masked_mae (label_start != NULL: y is the raw series).
 * partials: caller-owned scratch of batch*out_steps*MATGCN_METRIC_SUMS doubles; sums: out_steps*MATGCN_METRIC_SUMS
 * doubles, overwritten, or added to when accumulate != 0 (several batches = one collect() over their concatenation,
 * which is how the executor evaluates, :289).  Fixed summation order: run-to-run identical. */
#define MATGCN_METRIC_SUMS 14
#define MATGCN_METRICS 10 /* MAE, MAPE, MSE, RMSE, masked_MAE, masked_MAPE, masked_MSE, masked_RMSE, R2, EVAR */
typedef struct matgcn_metric_scale {
  const float* mean;   /* device: 1 value, or N with per_node; NULL (with std) = identity */
  const float* std;
  int32_t per_node;
  const float* mean2;  /* device (N) or NULL: second, per-node affine (group-std re-transform) */
  const float* std2;
  float clamp_min;     /* NaN: off */
  float truth_min;     /* NaN: off */
  float min_s;         /* < 0: off */
} matgcn_metric_scale;
int matgcn_metric_sums(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                       int out_dim, int y_steps, int y_feat, int y_start, const matgcn_metric_scale* scale,
                       double* partials, double* sums, int accumulate, void* stream);
/* table (2, out_steps, MATGCN_METRICS) doubles, device: [0] "single" mode (horizon o alone), [1] "average" mode
 * (horizons 0..o), metric order as MATGCN_METRICS above (= TrafficStateEvaluator.json).  swap_r2 != 0: R2 / EVAR with
 * prediction and truth exchanged, the way traffic_state_executor.py:318-319 calls sklearn. */
int matgcn_metric_table(const double* sums, int out_steps, int swap_r2, double* table, void* stream);

/* The same 14 sums grouped per horizon AND node - the tract-by-tract view of result_plot.py:102-134 without a row per
 * prediction element.  Per-element terms, descriptor, geometry, labels and series handling are those of
 * matgcn_metric_sums (out_steps in 1 .. 64; series rows clamped and counted); sums is (out_steps, nodes,
 * MATGCN_METRIC_SUMS) doubles and entry [o][n] sums over the batch rows b and the out_dim channels c in a FIXED ORDER:
 * start from the stored value when accumulate != 0, else from 0, and add the terms one at a time in ascending (b, c).
 * So one call over B samples and several accumulating calls over the same samples in the same order give identical
 * bits for any finite input, and nothing depends on the order workgroups run in.  One launch: a thread owns one
 * (horizon, node) and walks the batch itself, so there is no stage-1 scratch - matgcn_metric_sums_nodes_bytes reports 0
 * today and callers size `scratch` by it (NULL is accepted while it is 0; a smaller buffer is
 * MATGCN_ERR_SMALL_BUFFER).  Nothing is allocated, no atomics, the caller's stream only, every argument checked on the
 * host before the launch. */
int matgcn_metric_sums_nodes_bytes(int batch, int out_steps, int nodes, int out_dim, size_t* bytes);
int matgcn_metric_sums_nodes(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps,
                             int nodes, int out_dim, int y_steps, int y_feat, int y_start,
                             const matgcn_metric_scale* scale, void* scratch, size_t scratch_bytes,
                             double* sums /* (out_steps, nodes, MATGCN_METRIC_SUMS) */, int accumulate, void* stream);
/* table (rows, MATGCN_METRICS) doubles, device: row r from sum_{f < fold} sums[f*rows + r][:], added in ascending f from
 * 0, with exactly the arithmetic of the "single" table of matgcn_metric_table (one device function; on the same 14 sums
 * the same bits, zero counts included).  fold = 1, rows = out_steps*nodes: the table per horizon and node; fold =
 * out_steps, rows = nodes: the table per node over all horizons - the tract ranking.  rows, fold >= 1. */
int matgcn_metric_table_rows(const double* sums, int rows, int fold, int swap_r2, double* table, void* stream);

/* ---- training step: forward that keeps activations + backward -----------
 * Replaces torch autograd through MultiATGCN.forward as driven by TrafficStateExecutor._train_epoch
 * (libcity/executor/traffic_state_executor.py:411-422: loss = calculate_loss(batch); loss.backward()).
 * matgcn_grads mirrors matgcn_params field by field (same shapes); every non-NULL gradient is OVERWRITTEN.
 * node_emb may be NULL (node_specific_off freezes it); node_vec1/2 are required iff adp_mode == UNI.
 * `train` is one more caller-owned device buffer of matgcn_train_bytes(): forward_train saves z, r, hc of the
 * graph cell, z2, r2, hc2 of the residual cell, the initial state and the graph-mixed rows of every (layer, step) into it, backward uses
 * the rest as scratch.  matgcn_backward must see the SAME workspace and train buffers, untouched, that the matching
 * matgcn_forward_train call used (the sequences of every layer live in the workspace).
 * d_out (B, output_window, N, output_dim) is the gradient of the loss w.r.t. the forward's output.
 * drop_mask: NULL (eval-mode forward), or the training-mode dropout in front of end_conv (MultiATGCN.py:416,
 * F.dropout p = 0.1) as a (B, T, N, H) device tensor of multipliers 0 or 1/(1-p) drawn by the caller's RNG
 * (torch: F.dropout(torch.ones(B,T,N,H))); the same mask goes to the matching matgcn_backward.
 * Reductions that meet in one address: by default fp32 atomics - gradients are reproducible to rounding, not bitwise;
 * with matgcn_set_deterministic(1) in a fixed order - gradients are bit-identical from run to run (see there).
 * With gcn_off the dense cells' nn.Linear gradients come back in res_gate / res_update (as their weights go in);
 * with fnn_off drop_mask is (B, 1, N, H). */
typedef struct matgcn_agcn_grads {
  float* weights_g;
  float* weights_pool;
  float* bias_pool;
} matgcn_agcn_grads;

typedef struct matgcn_linear_grads {
  float* weight;
  float* bias;
} matgcn_linear_grads;

typedef struct matgcn_grads {
  float* node_emb;
  float* node_vec1;
  float* node_vec2;
  float* static_supports; /* unused: the static supports are constants */
  float* weight_tsg;
  float* weight_ts[MATGCN_MAX_HEADS];
  float* weights_gru;
  matgcn_agcn_grads gate[MATGCN_MAX_LAYERS];
  matgcn_agcn_grads update[MATGCN_MAX_LAYERS];
  matgcn_linear_grads res_gate[MATGCN_MAX_LAYERS];
  matgcn_linear_grads res_update[MATGCN_MAX_LAYERS];
  float* end_conv_weight;
  float* end_conv_bias;
} matgcn_grads;

int matgcn_train_bytes(const matgcn_dims* dims, size_t* bytes);
/* src != NULL: the batch comes from the device-resident series (X is ignored and may be NULL), as in
 * matgcn_forward_series; the matching matgcn_backward must get the same descriptor. */
int matgcn_forward_train(const matgcn_dims* dims, const matgcn_params* params, const void* prepared,
                         const float* X, const matgcn_series* src, const float* h0, const float* drop_mask, float* out,
                         void* workspace, size_t workspace_bytes, void* train, size_t train_bytes, void* stream);
/* h0: the pointer the matching matgcn_forward_train saw (NULL = zero initial state; the backward reads the padded copy
 * forward_train kept in `train`, the pointer only says that there was one).  d_h0: (L, B, N, H) gradient of the loss
 * w.r.t. the initial state, or NULL when the caller does not need it (it is overwritten, not accumulated). */
int matgcn_backward(const matgcn_dims* dims, const matgcn_params* params, const void* prepared, const float* X,
                    const matgcn_series* src, const float* h0, const float* drop_mask, const float* d_out,
                    const matgcn_grads* grads, float* d_h0, void* workspace, size_t workspace_bytes, void* train,
                    size_t train_bytes, void* stream);

/* The one contraction kernel of the backward, exposed for its parity test: a strided, two-level-batched fp32
 * GEMM  C[b1][b2] (+)= alpha * sum_{k2,k} A[b1][b2][m][k2][k] B[b1][b2][k2][k][n].  desc (22 x int64, host):
 * M, N, K, K2, sAm, sAk, sAk2, sBk, sBn, sBk2, sCm, sCn, nb1, nb2, bA1, bA2, bB1, bB2, bC1, bC2,
 * mode (0: C = alpha*acc + beta*C; 1: atomic add into C), split (K ranges per output tile, mode 1). */
int matgcn_debug_gemm(const float* A, const float* B, float* C, const int64_t* desc, float alpha, float beta,
                      void* stream);

/* ---- device-side dropout: seeded training masks and Monte-Carlo-dropout forecasts --------------------------------------
 * The dropout in front of end_conv (MultiATGCN.py:416) drawn INSIDE the kernels that apply it, from a counter-based
 * generator, so that no mask tensor exists anywhere: the descriptor below stands for a (B, headT, N, 64) tensor of
 * multipliers 0 or 1/(1-p) - headT = T, or 1 with fnn_off; 64 is the kernel-visible width, zero-padded models included -
 * that the library never materialises (matgcn_dropout_mask writes it out for whoever wants to look).
 * Generator: Philox4x32-10 (Random123; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85).
 *   key = (lo32(seed), hi32(seed));  counter = (lo32(q), hi32(q), lo32(offset), hi32(offset)),  q = idx >> 2,
 *   idx = ((b*headT + t')*N + n)*64 + h the element's position in the logical mask - independent of the padded node
 *   count, tiles, row variants and schedule;  output word idx & 3 decides element idx:  kept iff word >= thr,
 *   thr = floor((double)p * 2^32) (p = 0.1f: 429496736);  a kept element is multiplied by (float)(1.0 / (1.0 - (double)p)),
 *   a dropped one by 0.  Monte-Carlo sample s of matgcn_forward_mc draws with offset + s.
 * A host struct, read at call time; 0 <= p < 1, anything else (NaN included) is MATGCN_ERR_BAD_ARG.  A training loop
 * advances `offset` by one per step; ranks of a data-parallel job use disjoint offset ranges. */
typedef struct matgcn_dropout {
  uint64_t seed;
  uint64_t offset;
  float p;
} matgcn_dropout;

#define MATGCN_MAX_MC_SAMPLES 1024

/* Writes the (B, headT, N, 64) mask the descriptor stands for (for tests, and for callers that want to look at it). */
int matgcn_dropout_mask(const matgcn_dims* dims, const matgcn_dropout* dropout, float* mask, void* stream);

/* matgcn_forward_train / matgcn_backward with the descriptor in place of drop_mask (NULL = no dropout).  Bit for bit
 * what the unseeded pair gives on the mask matgcn_dropout_mask writes for the same descriptor - `out`, the saved
 * activations, and with matgcn_set_deterministic(1) every gradient - without the tensor: graph models draw in the top
 * layer's update kernel as it stores the sequence (the SEED instantiations of k_update16), gcn_off models in one
 * element-wise pass (k_apply_dropout), and the backward draws again in the epilogue of the head's data gradient
 * (k_bgemm<BG_HEAD_SEED>).  The backward must get the descriptor its forward got, as it must get the same mask tensor
 * today.  Every setting (training precision, three-piece training, deterministic, wavefront) applies as to the unseeded
 * pair; matgcn_train_bytes and matgcn_workspace_bytes are unchanged.
 * Measured at Baltimore 403 / B = 64 (MI355X, tools/train_step.py [--device-dropout] bm403 33, one box and one session, the
 * parent build, this build and this build seeded alternating twice, median of 30 steps each): seeded
 * training step 21.47 / 21.41 ms, forward_train 7.59 / 7.48, backward 13.74 / 13.78 - against the parent's step with torch
 * drawing the mask 21.45 / 21.63 ms (7.71 / 7.58, 13.57 / 13.91) and this build's unseeded step 21.58 / 21.55 ms: all three
 * level within run-to-run noise; no speed-up is claimed, the mask tensor (158 466 048 bytes at this shape) is what goes. */
int matgcn_forward_train_seeded(const matgcn_dims* dims, const matgcn_params* params, const void* prepared, const float* X,
                                const matgcn_series* src, const float* h0, const matgcn_dropout* dropout, float* out,
                                void* workspace, size_t workspace_bytes, void* train, size_t train_bytes, void* stream);
int matgcn_backward_seeded(const matgcn_dims* dims, const matgcn_params* params, const void* prepared, const float* X,
                           const matgcn_series* src, const float* h0, const matgcn_dropout* dropout, const float* d_out,
                           const matgcn_grads* grads, float* d_h0, void* workspace, size_t workspace_bytes, void* train,
                           size_t train_bytes, void* stream);

/* Monte-Carlo dropout: the eval-mode encoder ONCE - the kernels and the precision mode of matgcn_forward /
 * matgcn_forward_series (src != NULL: the batch comes from the series, X is ignored) - then the head over `samples`
 * masks (1 .. MATGCN_MAX_MC_SAMPLES, else MATGCN_ERR_BAD_ARG) in one launch (k_head_mc): sample s is the head of
 * seq * mask(seed, offset + s), with k_head's reduction order - bit-equal to matgcn_output_head on that product.
 * mean, std: (B, out, N, od); std is the POPULATION standard deviation over the samples, formed around a running mean
 * (Welford) in fp32 - exactly 0 for samples == 1.  samples_out: (samples, B, out, N, od), or NULL.
 * The head's 24 steps of a (b, 32-node) tile stay in registers over all samples (6 steps x 8 float4 per lane, one wave
 * per SIMD): in_steps > 24 without fnn_off returns MATGCN_ERR_UNSUPPORTED.  Workspace as matgcn_forward.
 * Measured at Baltimore 403 / B = 64 (MI355X, tools/mc_time.py bm403 20 32 128, median of 20 calls, HIP events): 9.09 ms at
 * S = 32 and 16.85 ms at S = 128 against 6.46 ms for one matgcn_forward of the same process - 81-82 us per sample (S
 * host-loop forwards: 207 / 827 ms).  k_head_mc's own duration under a kernel trace has NOT been measured yet (DESIGN.md
 * section 5d says why, and that its register budget must be re-read from the ISA after a compiler change). */
int matgcn_forward_mc(const matgcn_dims* dims, const matgcn_params* params, const void* prepared, const float* X,
                      const matgcn_series* src, const float* h0, const matgcn_dropout* dropout, int samples, float* mean,
                      float* std, float* samples_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- prediction intervals and probabilistic scores from the Monte-Carlo-dropout samples ----------------------------------
 * Both entry points read the sample-major tensor matgcn_forward_mc writes to samples_out: samples (S, E), E = B*out*N*od,
 * S = n_samples in 1 .. MATGCN_MAX_MC_SAMPLES.  A workgroup takes a tile of consecutive elements and all S samples of each
 * (every sample row is read from HBM once), de-scales on load, p = x*std + mean as an fp32 product and an fp32 sum (two
 * roundings, never fused), and sorts every element's column x(0) <= .. <= x(S-1) in LDS (bitonic network over S rounded
 * up to a power of two; the padding never reaches a result).  Tile: 64 elements up to S = 256, 32 up to 512, 16 up to 1024
 * (at most 64 KB of LDS).  Nothing is allocated, no atomics, work on the caller's stream only, fixed summation order:
 * results are run-to-run identical and independent of the order the workgroups run in.
 * Samples are assumed finite.  A non-finite sample (NaN, +-inf) causes no out-of-bounds access and no hang, but the
 * results of its element - and the sums that element enters - are UNSPECIFIED.  The sign of a zero result is unspecified.
 *
 * Quantile of level q (probs: HOST array of n_probs floats, 1 .. MATGCN_MAX_MC_QUANTILES of them, each in [0, 1], ascending;
 * anything else, NaN included, is MATGCN_ERR_BAD_ARG): the host forms h = (double)q*(S-1), j = floor(h), g = (float)(h-j);
 * the device Q = lo + g*(hi - lo) with lo = x(j), hi = x(min(j+1, S-1)), three fp32 roundings - numpy's default "linear"
 * rule, reproduced bit for bit by numpy float32 arithmetic.  Level 0 is the minimum and level 1 the maximum, exactly.
 * quantiles: (n_probs, E), device. */
#define MATGCN_MAX_MC_QUANTILES 8
#define MATGCN_MC_SCORE_SUMS 5            /* + one pinball sum per level */
int matgcn_mc_quantiles(const float* samples, int n_samples, int64_t elems, const float* probs /*HOST*/, int n_probs,
                        float mean, float std, float* quantiles /* (n_probs, elems) */, void* stream);

/* Scores of the ensemble against the labels, per horizon, for a whole test set batch by batch.  Labels, mask and
 * geometry as matgcn_masked_mae: l = y*std + mean (two fp32 roundings); l := 0 where |l| < min_s (min_s < 0: off);
 * mask = (l != null_val), with a NaN null_val mask = !isnan(l); y (B, y_steps >= out, N, y_feat), channels y_start ..
 * y_start+od-1, or - label_start != NULL (device, B int32) - the raw series (y_steps, N, y_feat) whose rows
 * label_start[b] + o are sample b's targets (rows outside the series are clamped and counted: matgcn_series_violations).
 * Per unmasked element, in fp64 from the fp32 values (Q_k the quantile of level k, first / last = the outer two levels):
 *   CRPS    = (1/S) sum_i |x(i) - l| - (1/S^2) sum_i (2i - S + 1) x(i)        (= mean|x - l| - mean|x - x'| / 2)
 *   covered = 1 iff Q_first <= l <= Q_last, compared in fp32;    width = Q_last - Q_first
 *   Winkler = width + (2/alpha) max(Q_first - l, 0) + (2/alpha) max(l - Q_last, 0),  alpha = 1 - ((double)q_last -
 *             (double)q_first); for alpha = 0 the width alone
 *   pinball_k = max(q_k (l - Q_k), (q_k - 1)(l - Q_k))
 * sums (out_steps, 5 + n_probs) doubles, device: [count, sum CRPS, sum covered, sum width, sum Winkler, sum pinball_0 ..],
 * overwritten, or added to when accumulate != 0 (several batches = one call over their concatenation).  A tile never
 * straddles two (b, horizon) rows; stage 1 writes one partial per workgroup into `scratch` (caller-owned device memory of
 * matgcn_mc_scores_bytes bytes, less is MATGCN_ERR_SMALL_BUFFER; contents before and after are of no interest), stage 2 adds
 * them in ascending index.  Every argument is checked on the host before anything is launched.
 * Measured at Baltimore 403 / B = 64 (MI355X, tools/mc_scores_time.py, median of 20 calls, HIP events; DESIGN.md section
 * 5d): S = 32 (79 MB of samples): matgcn_mc_quantiles (three
 * levels) 0.122 ms, matgcn_mc_scores 0.235 ms, torch.sort + the same interpolation 0.391 ms, one read of the tensor
 * (samples.sum(0)) 0.019 ms;  S = 128 (317 MB): 0.828 / 1.044 / 4.760 / 0.058 ms.  Faster than the torch route (3.2x and
 * 5.7x for the quantiles) and 6 to 14 times the single read: the kernels are bound by the LDS passes of the sorting
 * network (one barrier per stage), not by HBM. */
int matgcn_mc_scores_bytes(int batch, int out_steps, int nodes, int out_dim, int n_samples, int n_probs, size_t* bytes);
int matgcn_mc_scores(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch,
                     int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean, float std,
                     float null_val, float min_s, const float* probs /*HOST*/, int n_probs, void* scratch,
                     size_t scratch_bytes, double* sums /* (out_steps, 5 + n_probs) */, int accumulate, void* stream);

/* Both on the re-transformed scale, per node.  The descriptor is the matgcn_metric_scale of the metric sums: every
 * sample - and in the scores the label - takes its first affine (scalar, or one pair per node: per_node; NULL =
 * identity) and then the per-node second affine, each an fp32 product plus an fp32 sum, never fused; samples below
 * clamp_min are set to it BEFORE the sort (the executor's prediction_t < 0 -> 0; NaN: off).  Sort, quantile rule and
 * roundings are those above.
 *
 * matgcn_mc_quantiles_scaled: matgcn_mc_quantiles with the descriptor; element g of the (.., nodes, out_dim) tensor
 * belongs to node (g / out_dim) % nodes, elems is a multiple of nodes*out_dim.  truth_min and min_s are not used.  With
 * a scalar affine and no clamp: the bits of matgcn_mc_quantiles.
 *
 * matgcn_mc_scores_nodes: the score terms of matgcn_mc_scores (same formulas and roundings) grouped per horizon and
 * node: sums (out_steps, nodes, 5 + n_probs) doubles, out_steps in 1 .. 64.  Elements with l <= truth_min are left out
 * (NaN: off; tested before min_s); l := 0 where |l| < min_s and the null_val mask as in matgcn_mc_scores.  Entry [o][n]
 * starts from the stored value when accumulate != 0, else from 0, and adds the terms of its elements one at a time in
 * ascending (b, c): one call over B samples and accumulating calls over the same samples in pieces give identical bits.
 * With a scalar affine, no second affine, no clamp and no truth filter its rows added over the nodes are what
 * matgcn_mc_scores counts - identically in column 0, and in every column where all partial sums are exact.
 * Stage 1 sorts tile by tile as matgcn_mc_scores does (a tile spans several nodes, and with out_dim > 1 a node's
 * channels can sit in two tiles) and writes the terms of every element, zeros for a masked one, into `scratch`
 * (matgcn_mc_scores_nodes_bytes = 8*(5 + n_probs) bytes per element; less is MATGCN_ERR_SMALL_BUFFER; contents before
 * and after are of no interest); stage 2 owns one sum per thread.  Nothing is allocated, no atomics, the caller's stream
 * only, every argument checked on the host before anything is launched.
 * Measured at Baltimore 403 / B = 64 / out = 24 with the re-transform, clamp 0 and truth_min 6 (MI355X,
 * tools/node_scores_time.py, median of 20 calls, HIP events, one process; DESIGN.md sections 5b and 5d):
 * matgcn_metric_sums_nodes 0.048 ms (matgcn_metric_sums 0.049 ms, torch terms + index_add_ 0.342 ms);  S = 32:
 * matgcn_mc_scores_nodes 0.187 ms with 39.6 MB of scratch (matgcn_mc_scores 0.228 ms, torch.sort + terms + index_add_
 * 1.194 ms), matgcn_mc_quantiles_scaled 0.128 ms (matgcn_mc_quantiles 0.115 ms);  S = 128: 0.982 (1.042, 6.432) and 0.831
 * (0.817) ms.  The grouped forms were not slower than the per-horizon ones in this measurement. */
int matgcn_mc_quantiles_scaled(const float* samples, int n_samples, int64_t elems, int nodes, int out_dim,
                               const float* probs /*HOST*/, int n_probs, const matgcn_metric_scale* scale,
                               float* quantiles /* (n_probs, elems) */, void* stream);
int matgcn_mc_scores_nodes_bytes(int batch, int out_steps, int nodes, int out_dim, int n_samples, int n_probs,
                                 size_t* bytes);
int matgcn_mc_scores_nodes(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch,
                           int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start,
                           const matgcn_metric_scale* scale, float null_val, const float* probs /*HOST*/, int n_probs,
                           void* scratch, size_t scratch_bytes, double* sums /* (out_steps, nodes, 5 + n_probs) */,
                           int accumulate, void* stream);

/* ---- split conformal calibration of the band -----------------------------------------------------------------------------
 * The ensemble carries the head's uncertainty only, so its band [Q_first, Q_last] is too narrow.  Split conformal
 * calibration widens it by one rank statistic of held-out conformity scores per group, which gives the band's nominal
 * coverage on exchangeable data without retraining.  Three entry points: the scores of a batch, the margin per group from
 * a store of scores, and how often a margin held.  Nothing is allocated, no global atomics, no scratch, the caller's
 * stream only, every argument checked on the host before anything is launched; every result is run-to-run identical.
 *
 * matgcn_mc_conformity: arguments as matgcn_mc_scores_nodes (out_steps in 1 .. 64) with `scores` (B, out, N, od) floats
 * in place of scratch and sums; n_probs >= 2 (fewer is MATGCN_ERR_BAD_ARG).  Tile, sort, quantile rule, de-scaling of
 * label and samples, clamp, truth_min, min_s and the null_val mask are exactly those of matgcn_mc_scores_nodes.  Per
 * element the conformalized-quantile-regression score
 *   s = max(Q_first - l, l - Q_last),   each difference one fp32 rounding
 * (negative inside the band, 0 on its edge); a masked or filtered element stores a quiet NaN, so EVERY element of
 * `scores` is written.  Non-finite samples: as above, that element's score is unspecified.  A caller appends batch after
 * batch into a window-major store (rows_capacity, out, N*od) by passing store + rows_filled*out*N*od.
 *
 * matgcn_conformal_quantile: scores is such a store, (rows, out_steps, cols) with cols = N*od; rows beyond rows - 1 are
 * never read.  grouping 0: one group per horizon (margin, count: out_steps entries); grouping 1: one per (horizon,
 * column) (out_steps*cols entries).  Group g holds the non-NaN scores of its columns in rows 0 .. rows-1:
 *   n = their number;   k = max(1, ceil((double)(n + 1) * coverage)), one fp64 product;
 *   margin[g] = the k-th smallest of them when k <= n, else +inf (n = 0 included);   count[g] = n.
 * coverage in (0, 1], anything else (NaN included) is MATGCN_ERR_BAD_ARG; a caller calibrating the band of levels q_first,
 * q_last passes (double)q_last - (double)q_first, the convention of the Winkler score above.  The selection is exact: a
 * radix select over order-preserving 32-bit keys (u ^ 0xFFFFFFFF for negative floats, u | 0x80000000 otherwise; -0 sorts
 * before +0), four 8-bit passes over 256-bin histograms in LDS built with LDS integer adds, all four in one launch.
 * grouping 1: a workgroup owns 64 adjacent columns of one horizon (coalesced row reads, 64 x 256 bins = 64 KB);
 * grouping 0: one workgroup per horizon walks rows x cols.  Every loop bound is a host-known count and only integer
 * counts are accumulated, so no input value can change a trip count and no result depends on execution order.
 * Counts are 32-bit: rows (grouping 1) or rows*cols (grouping 0) of 2^31 - 4096 or more is MATGCN_ERR_UNSUPPORTED.
 *
 * matgcn_conformal_coverage: counts (groups, 2) int64 = [n, covered] per group of the same store and grouping, covered =
 * the non-NaN scores with s <= margin[g], compared in fp32 (a score equal to the margin is covered; under a +inf margin
 * every valid score is) - the coverage of the calibrated band in the conformal definition.  Overwritten, or added to
 * when accumulate != 0: a test split streamed batch by batch.  Integer sums only.
 * Argument checks of the last two: counts >= 1, out_steps in 1 .. 64, grouping in {0, 1}, non-null pointers,
 * rows*out_steps*cols within int64.
 * Measured at Baltimore 403 / B = 64 / out = 24 with the re-transform, clamp 0 and truth_min 6 (MI355X,
 * tools/conformal_time.py, one process, routes alternating three times, median of 20 calls, HIP events; DESIGN.md section
 * 5d.1): matgcn_mc_conformity 0.137 ms at S = 32 and 0.909 ms at S = 128 (matgcn_mc_scores_nodes 0.176 / 0.979 ms,
 * torch.sort + the same arithmetic 0.485 / 4.744 ms, same scores); on a store of 540 rows (20.9 MB)
 * matgcn_conformal_quantile 0.343 ms per horizon (torch.kthvalue per horizon, its rank read back each time: 19.96 ms)
 * and 0.224 ms per element (torch.sort per group 0.417 ms); matgcn_conformal_coverage over one batch 0.031 / 0.017 ms
 * (torch compare + sum 0.054 / 0.046 ms).  Every gap is above twice the spread of the visits (at most 0.009 ms). */
int matgcn_mc_conformity(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch,
                         int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start,
                         const matgcn_metric_scale* scale, float null_val, const float* probs /*HOST*/, int n_probs,
                         float* scores /* (batch, out_steps, nodes, out_dim) */, void* stream);
int matgcn_conformal_quantile(const float* scores, int64_t rows, int out_steps, int cols /* N*od */,
                              int grouping /* 0: per horizon, 1: per (horizon, column) */, double coverage,
                              float* margin /* (groups) */, int32_t* count /* (groups) */, void* stream);
int matgcn_conformal_coverage(const float* scores, int64_t rows, int out_steps, int cols, int grouping,
                              const float* margin /* (groups) */, int64_t* counts /* (groups, 2): n, covered */,
                              int accumulate, void* stream);

/* ---- totals over groups of nodes: regions (matgcn_regions.hip) -----------------------------------------------------------
 * Forecasts are made per node (census tract) and planned with per county, district or corridor.  Quantiles and errors do
 * not add, so the band and the scores of a region total are taken from totals formed sample by sample.  The two entry
 * points form them - of any (rows, nodes, out_dim) tensor (the point forecast, the Monte-Carlo-dropout samples) and of the
 * labels of a batch - on the re-transformed scale; every kernel above then applies to the result with nodes = n_groups and
 * an identity descriptor.
 *
 * matgcn_groups is a CSR list over groups: groups may overlap, nest, be empty or leave nodes out.  `ptr` is read on the
 * HOST at call time (ptr[0] = 0, non-decreasing, ptr[n_groups] = n_members, else MATGCN_ERR_BAD_ARG); the kernels read its
 * device copy.  Node indices are validated where the map is built; an index outside 0 .. nodes-1 is clamped into the row,
 * so no map makes a kernel read outside the tensor.
 *
 * Per member: value v of node n, channel c goes through the descriptor's first affine (scalar or per node; null =
 * identity), then its per-node second affine, each an fp32 product and an fp32 sum, never fused, as in
 * matgcn_mc_quantiles_scaled; then v := clamp_min where v < clamp_min (NaN: off).  truth_min and min_s are not used.
 * Per (row r, group g, channel c): start from 0.0 in fp64; for k = ptr[g] .. ptr[g+1]-1 in ascending k add
 * (double)weight[k] * (double)v(node[k]) (weight null = 1), one member at a time; round to fp32 once.  The product of
 * two fp32 values is exact in fp64, so a contracted fma gives the bits of multiply then add.  An empty group stores +0.0;
 * a NaN member makes the total NaN - the region-level mask: a region with a missing label has no label.
 * One thread owns a chain from end to end: no atomics, nothing allocated, the caller's stream only, EVERY element of
 * `out` is written, and the result does not depend on the order workgroups run in - the same bits every run, however a
 * test set is batched.  matgcn_group_sums reads each row once into an LDS tile (several rows in up to 32 KB, one long row
 * in up to 64 KB; a row of more than 16 383 floats is walked in global memory instead, same chain) and keeps a map of up
 * to 16 KB beside it.
 *
 * matgcn_group_label_sums reads labels under the label contract of matgcn_masked_mae: label_start null = window labels
 * (batch, y_steps, nodes, y_feat), channels y_start .. y_start + out_dim - 1 of steps 0 .. out_steps-1; otherwise `y` is
 * the raw series (y_steps, nodes, y_feat) and label_start (batch) its first label rows, clamped and counted through
 * matgcn_series_violations.
 * Argument checks, before any launch: non-null pointers (node may be null with n_members = 0); rows (batch, out_steps),
 * nodes, out_dim, n_groups >= 1, n_members >= 0; a lone mean or std; the label geometry; rows*n_groups*out_dim and
 * rows*nodes*out_dim within int64 - MATGCN_ERR_BAD_ARG.  nodes*out_dim or 256*n_groups*out_dim of 2^31 or more, or more
 * than 2^31 - 1 workgroups, is MATGCN_ERR_UNSUPPORTED.
 * Measured at Baltimore 403 / B = 64 / out = 24 with the re-transform and clamp 0 (MI355X, tools/region_time.py, one
 * process, routes alternating three times, median of 20 calls, HIP events), ten regions / the same
 * plus one whole-city group: matgcn_group_sums 0.078 / 0.124 ms at S = 32 and 0.248 / 0.396 ms at S = 128; torch de-scale +
 * clamp + matmul with the dense membership matrix 0.146 / 0.145 and 0.614 / 0.614 ms; torch index_add_ 1.62 / 3.11 and
 * 5.79 / 11.9 ms; one plain read of the samples 0.019 and 0.057 ms.  Every gap to the matmul route is above twice the
 * spread of the visits (at most 0.005 ms); the kernel is 4.1 to 7.0 times the plain read: not at memory speed. */
typedef struct matgcn_groups {
  const int32_t* ptr;     /* HOST, n_groups + 1 entries, ptr[0] = 0, non-decreasing, ptr[n_groups] = n_members */
  const int32_t* ptr_dev; /* device copy of ptr */
  const int32_t* node;    /* device, n_members node indices in 0 .. nodes-1, in the order they are to be added */
  const float*   weight;  /* device, n_members, or NULL = 1 */
  int32_t n_groups, n_members;
} matgcn_groups;
int matgcn_group_sums(const float* values, int64_t rows, int nodes, int out_dim, const matgcn_metric_scale* scale,
                      const matgcn_groups* groups, float* out /* (rows, n_groups, out_dim) */, void* stream);
int matgcn_group_label_sums(const float* y, const int32_t* label_start, int batch, int out_steps, int nodes, int out_dim,
                            int y_steps, int y_feat, int y_start, const matgcn_metric_scale* scale,
                            const matgcn_groups* groups, float* out /* (batch, out_steps, n_groups, out_dim) */,
                            void* stream);

/* ---- a training objective on region totals, value and gradient (matgcn_region_loss.hip) ------------------------------------
 * Still ABI 12: new names only.  Training on  tract_weight * L(tracts) + region_weight * L(region totals):  the first term
 * is matgcn_loss / matgcn_loss_grad, the second this pair, with any of the seven kinds.
 * Inputs: pred (B, out, N, od), labels with the geometry of matgcn_loss, a matgcn_loss_desc, and the region map in two
 * forms: by group (the matgcn_groups of matgcn_group_sums) and, for the gradient, by node (below).
 * Totals.  P = matgcn_group_sums(pred), L = matgcn_group_label_sums(y), both with the descriptor's scalar (mean, std) as the
 * first affine, no second affine and no clamp: the bits of those entry points, fp32, (B*out, G, od), kept in scratch.
 * Value.  matgcn_loss on (P, L) with nodes = G, an identity affine (mean 0, std 1) and the descriptor's kind, null_val,
 * min_s and delta: result[0] the objective over all horizons, result[1 + k] horizon k - bit for bit the composition of the
 * three entry points.  Masking therefore acts on totals: a region whose label total is NaN (any NaN member) is left out
 * under the NaN-null kinds; under null_val = 0 a region is zeroed and masked only when its TOTAL is below min_s; a masked
 * tract simply adds its value to its regions.
 * Gradient.  Per region element (r, g, c): q = fp32(slope * keep), slope = dt/dp of the table above at (P, L, d = P - L);
 * q = 0 where the forward replaced a NaN term by 0; RMSE: q divided by 2 rmse, every q = 0 when rmse == 0 - the g of
 * matgcn_loss_grad before its final scaling, rounded to fp32 ONCE.  The rounding is deliberate: (double)w * (double)q is
 * then exact in fp64, so a contracted fma gives the bits of multiply then add (the idiom of matgcn_group_sums) and no
 * compiler flag decides the result.  Per tract element (r, n, c): acc = 0.0 in fp64; for each membership of node n, in
 * ascending member position k of the by-group map, acc += (double)weight[k] * (double)q[r, group[k], c] (weight null = 1);
 * part = ((double)upstream[0] * (double)std) * acc / cnt, where cnt is the kept count the value call left in scratch
 * (masked kinds) or B*out*G*od (the others), and cnt == 0 gives part = 0;  d_pred = fp32(part), or with a non-null base
 * d_pred = fp32((double)base + part).  base has the shape of d_pred and may alias it.  A node in no region gets base's
 * bits, or +0.0 without a base.  EVERY element of d_pred is written.
 * One thread owns a chain from end to end: no atomics, nothing allocated, the caller's stream only, and the result does
 * not depend on the order workgroups run in - the same bits every run.  The gradient reads pred and y only through the
 * totals in scratch: it touches scratch, the by-node map, base, d_pred and upstream.  A workgroup computes the q of a tile
 * of rows into LDS (at most 8192 floats) and keeps a by-node map of up to 16 KB beside them; with G * out_dim above 8192
 * the coefficients are recomputed per membership from the totals in global memory instead: same chain, same bits.
 * by_node is the transposed map in the same struct: n_groups = nodes, ptr (nodes + 1 entries, read on the HOST and checked
 * like the by-group ptr; its last entry must equal by_group->n_members), node[e] a GROUP index (clamped into 0 .. G-1 in
 * the kernel, as the forward clamps node indices), weight[e] that membership's weight (null with a null by-group weight);
 * the entries of a node in ascending member position of the by-group map.  The library does not verify that the two maps
 * agree: regions.RegionMap builds one from the other.
 * scratch: caller-owned, 8-byte aligned device memory of matgcn_region_loss_bytes: the two total tensors, matgcn_loss's own
 * scratch for (B, out, G, od), then the descriptor's (mean, std) as two floats where the total kernels read them.  The
 * gradient call takes the scratch its value call left, like matgcn_loss_grad; every word read is written first by the same
 * pair of calls.
 * Argument checks, before any launch, as matgcn_loss and matgcn_group_sums: null pointers MATGCN_ERR_NULL; geometry
 * (out_steps in 1 .. 64), kind, delta, either map's ptr, a misaligned scratch, a by_node whose n_groups is not `nodes` or
 * whose member count differs - MATGCN_ERR_BAD_ARG; a short scratch MATGCN_ERR_SMALL_BUFFER; index spaces of 2^31 or more
 * MATGCN_ERR_UNSUPPORTED.
 * Measured at Baltimore 403 / B = 64 / out = 24, tract weight 1, region weight 0.5 (MI355X, tools/region_loss_time.py, one
 * process, routes alternating three times, median of 30 steps, HIP events), ten regions / the same
 * plus one whole-city group, forward + backward of the loss alone over masked_mae, huber, masked_mse: the four calls of
 * both levels behind ops.tract_region_loss 0.285-0.289 / 0.286-0.290 ms; torch de-scale + dense-membership matmul + closure
 * arithmetic + autograd on both levels 0.747-0.789 / 0.767-0.794 ms (spread at most 0.048 ms: every gap is above twice it);
 * the tract-level pair alone 0.177-0.184 ms - all host-bound (the enqueue time is within 0.007 ms of the device time).
 * matgcn_region_loss_grad alone 0.0158-0.0161 ms against 0.0095-0.0097 ms for one plain read of the totals plus one write
 * of d_pred: 1.65x to 1.68x, not at memory speed.  The whole training step 21.80 / 21.86 ms with the region term against
 * 21.63 / 21.60 ms without: about 1 % more, not level. */
int matgcn_region_loss_bytes(int batch, int out_steps, int n_groups, int out_dim, size_t* bytes);
int matgcn_region_loss(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                       int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc,
                       const matgcn_groups* by_group, void* scratch, size_t scratch_bytes,
                       float* result /* 1 + out_steps */, void* stream);
int matgcn_region_loss_grad(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps,
                            int nodes, int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc,
                            const matgcn_groups* by_group, const matgcn_groups* by_node, const void* scratch,
                            size_t scratch_bytes, const float* upstream, const float* base /* or NULL */, float* d_pred,
                            void* stream);

/* ---- the optimizer step: global gradient norm, clip and Adam over a table of tensors -------------------------------------
 * What clip_grad_norm_(params, max_norm) followed by torch.optim.Adam.step() does (no amsgrad, no maximize), as three
 * launches over every tensor at once.  The tensors are described by a HOST array of matgcn_opt_tensor, read at call time;
 * every pointer in it is DEVICE fp32, contiguous, at any 4-byte alignment (float4 accesses where all four pointers of a
 * tensor are 16-byte aligned, scalar ones otherwise - the same bits either way).  numel == 0 is allowed and skipped (its
 * pointers are not looked at); matgcn_grad_norm* read `grad` and `numel` only.
 * Nothing is allocated, work runs on the caller's stream only, no atomics, no host synchronisation, and every argument is
 * checked on the host before anything is launched.  `grad` is NEVER written: unlike clip_grad_norm_, which scales the
 * .grad tensors in place, the clip coefficient is applied as the gradients are read, and they keep their unclipped values.
 * Gradients are assumed finite.  A non-finite one causes no out-of-bounds access and no hang; the results are UNSPECIFIED.
 *
 * Norm.  The index space is cut into chunks of 4096 elements that never straddle two tensors (each tensor is rounded up to
 * whole chunks).  Launch 1: one workgroup per chunk squares and sums its elements in fp64 in a fixed in-workgroup order
 * and writes one double per chunk into `scratch` (caller-owned device memory of matgcn_grad_norm_bytes = 8 bytes per chunk,
 * less is MATGCN_ERR_SMALL_BUFFER; contents before and after are of no interest).  Launch 2: one workgroup adds the
 * partials in ascending index in fp64 and stores total_norm = (float)sqrt(sum).  The squares are exact in fp64 and the sum
 * carries 29 bits more than the result: the norm is the correctly rounded fp32 value up to one ulp, run-to-run identical
 * and independent of the order the workgroups run in (and of the alignment of the tensors).
 *
 * Update.  Launch 3, one per at most 64 tensors: the table travels by value in the kernel arguments, so no device copy of
 * it exists and nothing is uploaded per step; more tensors are more launches of the same kernel (of launch 1 likewise).
 * Per element, one rounding per operation, never fused, `/` and sqrt correctly rounded - the order of torch's
 * _single_tensor_adam:
 *   coef = max_norm > 0 ? min(1, max_norm / (total_norm + 1e-6)) : 1        (a NaN norm gives a NaN coef, as torch's clamp)
 *   g = grad * coef;   if (weight_decay != 0) g = g + weight_decay * p       (torch Adam's L2 form)
 *   m = (float)(m + (1 - beta1) * (g - m))
 *   v = (float)(beta2 * v + ((1 - beta2) * g) * g)
 *   p = p - step_size * (m / (sqrt(v) / sqrt(bc2) + eps)),   step_size = lr / bc1, bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
 * coef, g and the two moment lines are evaluated in fp64 from the fp32 values, with 1 - beta1, 1 - beta2, beta2 and
 * weight_decay as doubles, and each moment is rounded to fp32 once: coef is common to all elements and g enters v squared,
 * so an fp32 coef would put its one rounding, doubled, into every v at once - measured against torch's own float64 run,
 * the all-fp32 form of these lines left the margin the tests give (twice the gap of torch's float32 run) in 6 % of random
 * clipped one-step cases, this form in none.  The last line runs in fp32 on the rounded moments, exactly as torch's does;
 * step_size and sqrt(bc2) are formed on the host in double and rounded once.  Each float
 * of matgcn_adam is read as the shortest decimal that rounds to it (0.999f as 0.999, what a caller wrote and what Python
 * holds): 1 - beta2 is then torch's 1e-3, not the 0.99998713e-3 the float's own value would give.
 * matgcn_adam is a host struct, read at call time.  MATGCN_ERR_BAD_ARG: n < 1, a numel < 0, lr / eps / weight_decay
 * negative or NaN, beta1 or beta2 outside [0, 1), step < 1, max_norm NaN.  MATGCN_ERR_NULL: t, hp, a pointer of a tensor
 * with numel > 0, total_norm of matgcn_grad_norm, or total_norm of matgcn_adam_step while max_norm > 0 (with max_norm <= 0
 * it is not read and may be NULL).  Tensors whose step counts differ go into separate calls. */
typedef struct matgcn_opt_tensor {   /* HOST array element; all pointers DEVICE fp32, contiguous */
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t numel;
} matgcn_opt_tensor;
typedef struct matgcn_adam {         /* host struct, read at call time */
  float lr, beta1, beta2, eps, weight_decay;  /* weight_decay: torch Adam's L2 form (g += wd*p), 0 = off */
  float max_norm;                              /* > 0: clip to this global norm; <= 0: no clipping */
  int64_t step;                                /* 1-based step count after this update */
} matgcn_adam;

int matgcn_grad_norm_bytes(const matgcn_opt_tensor* t, int n, size_t* bytes);
int matgcn_grad_norm(const matgcn_opt_tensor* t, int n, void* scratch, size_t scratch_bytes,
                     float* total_norm /* device, 1 float */, void* stream);
int matgcn_adam_step(const matgcn_opt_tensor* t, int n, const matgcn_adam* hp,
                     const float* total_norm /* device; required iff max_norm > 0 */, void* stream);

/* ---- scheduling option ------------------------------------------------------------------------
 * The encoder runs the recurrent chains of the layers as a wavefront on internal HIP streams (created once, on
 * first use; forked from and joined back into the caller's stream with events, so the caller still sees one
 * in-order stream).  matgcn_set_wavefront(0) serialises everything on the caller's stream instead - same kernels,
 * same results; used to time one kernel alone.  (A lock-step pairing of the chains through per-kernel events was
 * measured and rejected: the cross-stream waits cost more than the pairing gains.)  Any non-zero value selects the
 * wavefront.  Returns the previous setting. */
int matgcn_set_wavefront(int enabled);

/* Hardware queues.  The HIP runtime maps the streams of a process onto GPU_MAX_HW_QUEUES (default 4) hardware queues per
 * stream priority, round robin in creation order, and which of the library's streams share a queue decides how well the
 * layers' chains overlap.  By default the library creates ordinary streams and runs the first chain on the caller's
 * stream: the best measured for a single process - but the pool is shared with every other stream of the process, and an
 * RCCL communicator created before the library's streams moves them onto each other's queues (forward 8.0 instead of
 * 6.8 ms at the headline shape, identical kernel durations: profiles/r04_rccl_queues_lab.log).
 * matgcn_set_stream_pool(1) - for data-parallel jobs - makes the library create its streams at the device's highest
 * priority (a queue pool nothing else in the process uses) at chosen places of the round robin, and run
 * matgcn_forward / _forward_series / _forward_train / _backward on a library stream forked from and joined back into the
 * caller's: the same timings with and without a process group, about 1 % behind the default without one.  Must be called
 * before the first of those entry points creates the streams (MATGCN_ERR_BAD_ARG afterwards, unless the mode asked for is
 * the one in use).  A scheduling change only: the forward's results are bit-identical in both modes, gradients agree up to the
 * order of the backward's atomic accumulations (as two runs in one mode do). */
int matgcn_set_stream_pool(int own);

/* Lazy prepare.  By default `prepared` is complete, in stream order, when matgcn_prepare returns.  With
 * matgcn_set_lazy_prepare(1) matgcn_prepare returns while the node-adaptive weight streams (most of its work) are still
 * being written on two library streams, and every entry point of this library that takes `prepared` orders its stream
 * behind them itself - the wavefront forward per layer: each chain waits for exactly the weights it reads, so the weight
 * preparation runs beside head fusion, the layer-0 fold and the first graph mix of matgcn_forward{,_series}.  A caller
 * that enables it promises (a) to keep `prepared` and the parameter tensors alive and unmodified until a later call of
 * this library THAT TAKES `prepared` (or matgcn_prepare_join) has been enqueued on the same stream - only those order
 * the stream behind the weight streams; the loss, metric, score, region and optimizer entry points do not -, and (b)
 * to call matgcn_prepare_join(stream) before it reads or frees `prepared` itself.  Meant for hosts that own `prepared`
 * for the lifetime of the model (the plugin class does).  (tests/test_stream_order.py holds both promises: the
 * parameters are overwritten right behind a forward that follows a lazy prepare, `prepared` behind the join.)
 * Both return MATGCN_OK / the previous setting. */
int matgcn_set_lazy_prepare(int enabled);
int matgcn_prepare_join(void* stream);

/* ---- precision option (BASELINE config 3's dtype; a side line, never the headline) -----------------------------
 * matgcn_set_mix_precision(1): the graph mixes of matgcn_forward / matgcn_forward_series round their operands - the
 * support stack and the state rows - to bf16 on the way into LDS and run on v_mfma_f32_16x16x16_bf16 with fp32
 * accumulation; inputs, outputs, the recurrent state, the node-wise contractions and everything in memory stay fp32.
 * matgcn_set_mix_precision(2): additionally the node-wise contractions of the recurrent step (MultiATGCN.py:108) and,
 * since round 4, of the hoisted x part of layers >= 1 take bf16 operands: the node-adaptive weights are streamed from a
 * bf16 copy of their fragment streams (made once per forward in the workspace - half the bytes of the largest stream of
 * a step), the rows [s | mix(s)] / [x | mix(x)] are rounded on their way into LDS, fp32 accumulation; the state, the
 * layer-0 x part, the residual cell and every epilogue stay fp32.
 * Both are NARROWER than the reference's fp32 arithmetic: measured max-normalised deviation from the fp32 path <= 3e-3
 * (mode 1) at N = 403 (tests/test_hip_parity.py::test_bf16_mix_variant holds both modes to 5e-3).  Governs
 * matgcn_forward / matgcn_forward_series only: matgcn_prepare and the unit entry points always use fp32 operands, the
 * training entry points follow matgcn_set_train_precision.
 * matgcn_set_mix_precision(3) ("bf16x3"): fp32 ACCURACY on the bf16 matrix instruction.  Every graph mix of
 * matgcn_forward / matgcn_forward_series - the recurrent step's two, the layer-0 fold, the hoisted x-part chunks - splits
 * both operands into three bf16 pieces, x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid),
 * and accumulates the six leading piece products (hi.lo, lo.hi, mid.mid, hi.mid, mid.hi, hi.hi, smallest first) in fp32 on
 * v_mfma_f32_16x16x32_bf16, with partial sums every 256 reduction indices past 1 024 nodes like the fp32 kernel.  Dropped:
 * mid.lo, lo.mid and lo.lo, each at most about 2^-24 relative.  The support stack is split once per forward into three
 * planes in the workspace (see matgcn_workspace_bytes), the state rows on their way into LDS.  Inputs, outputs, the
 * recurrent state, the node-wise contractions, the residual cell, matgcn_prepare, the unit entry points and everything in
 * memory stay fp32; modes 0, 1 and 2 keep their kernels and their bits.  Every mix of the two forwards has a mode-3
 * kernel (one 64 x 128 tile shape at every batch and graph size, odd batch sizes and the small batches of the fp32 path's
 * 64 x 32 tiles included), so no shape of the forwards falls back to an fp32 mix.  Training is a switch of its own,
 * matgcn_set_train_bf16x3 (below): matgcn_set_train_precision(3) means 0 and always will, so a process that sets only this
 * mode trains with the fp32 kernels and their bits.
 * Measured gap to the reference's float64 prediction (MI355X, tests/test_bf16x3.py, the bound is twice the reference's
 * own fp32-vs-float64 gap): bm403_out24 (N = 403, B = 4) worst element 3.87e-7, r.m.s. 4.91e-8 - the reference's own
 * fp32 run 4.45e-7 / 6.15e-8; synth4096_out24 (N = 4096, B = 2, partial sums) 2.66e-7 / 4.19e-8 - reference 4.69e-7 /
 * 5.83e-8.  At the seven shape-edge fixtures 4.1e-7 .. 6.4e-7 max-normalised from the float64 oracle (the fp32 path:
 * 4.0e-7 .. 8.2e-7; tolerance 1e-4).  Measured speed at Baltimore 403 / B = 64: step mix 33.0 us against 38.8 of the
 * fp32 kernel, forward 5.61 ms against 6.38.
 * Returns the previous setting; 0 (default) = fp32; any value other than 1, 2, 3 means 0. */
int matgcn_set_mix_precision(int mode);

/* Modes 1 and 2 for the training entry points (matgcn_forward_train, matgcn_backward); 0 (default) = fp32, any other
 * value - 3 included: three-piece training is a switch of its own, matgcn_set_train_bf16x3 - means 0; returns the previous setting.  The two settings are independent (a model can train in bf16 and
 * evaluate in fp32).
 *   matgcn_forward_train runs the kernels of the inference forward of that mode - mode >= 1: bf16 operands for the
 *   graph mixes (the mixed rows it saves for the weight gradients are their fp32 outputs); mode 2: also for the
 *   node-wise contractions of the recurrent step and of the hoisted x part of layers >= 1 (bf16 copies of the weight
 *   streams, made once per call in the workspace).  The saved activations, the state, the residual cell and every
 *   epilogue stay fp32.
 *   (fp32-accurate graph mixes on the bf16 instruction for training: matgcn_set_train_bf16x3, below.)
 *   matgcn_backward, mode >= 1: the transposed graph mixes (the chain's two per step and layer, the x columns of the
 *   last step and of layer 0) take bf16 operands with fp32 accumulation; mode 2: also the node-wise data-gradient
 *   contractions (the h columns of both AGCNs in the chain, the x columns of the layers), from bf16 copies of the plain
 *   folded weights that matgcn_forward_train makes in the train buffer.  Every parameter-gradient product, the
 *   gradients themselves and everything in memory stay fp32.
 * Contract between the two calls: matgcn_backward FOLLOWS the mode its matching matgcn_forward_train ran with (the library
 * remembers it per train buffer), whatever the setting is when the backward is called - a mode switch between the two
 * never mixes kernels of two modes.  A backward on a train buffer whose last forward_train failed returns
 * MATGCN_ERR_BAD_ARG; one the library has no record of runs with the current setting.
 * matgcn_workspace_bytes counts the bf16 weight-stream copies while either setting is 2; a mode-2 forward_train on a
 * workspace sized without them returns MATGCN_ERR_SMALL_BUFFER (ask again and re-allocate); likewise matgcn_train_bytes
 * counts the bf16 weight copies of the backward while matgcn_set_train_precision(2) is set, and a mode-2 forward_train /
 * backward on a train buffer without them returns MATGCN_ERR_SMALL_BUFFER.  Measured gap to the reference's autograd: <= 1.4e-2 max-normalised per gradient tensor
 * (tests/test_train_precision.py holds both modes to 2.7e-2; figures in DESIGN.md section 5). */
int matgcn_set_train_precision(int mode);

/* ---- three-piece training ("bf16x3" for the training entry points) ---------------------------------------------------
 * matgcn_set_train_bf16x3(1): the graph mixes of the training step - matgcn_forward_train's and the transposed ones of
 * matgcn_backward - take both operands as three bf16 pieces and accumulate the six leading piece products in fp32 on
 * v_mfma_f32_16x16x32_bf16, as matgcn_set_mix_precision(3) does for the inference forwards: fp32 accuracy, held to the fp32
 * path's own tolerances (1e-4 per gradient tensor against float64 autograd, tests/test_bf16x3_train.py).  Returns the
 * previous setting; 0 (default) = off; any non-zero value = on.  A symbol of its own, not a value of
 * matgcn_set_train_precision: ABI 12 defined every value of that setter outside 1 and 2 as 0.
 * Effective training mode, read by matgcn_forward_train on entry:
 *   matgcn_set_train_precision at 1 or 2 - that mode; this switch is ignored (the narrower arithmetic was asked for);
 *   matgcn_set_train_precision at 0 and this switch on - mode 3;
 *   otherwise - 0, fp32.
 * The library records mode 3 per train buffer like modes 1 and 2: matgcn_backward FOLLOWS the mode of its matching
 * matgcn_forward_train whatever the switch says when it is called; a backward on a train buffer the library has no
 * record of runs with the current effective mode.
 *   matgcn_forward_train, mode 3: the mixes of the inference forward of matgcn_set_mix_precision(3) (k_mix_bf16x3<0|1>,
 *   partial sums past 1 024 nodes); the support stack is split once per call into three planes in the workspace.  The
 *   mixed rows it saves are those kernels' fp32 outputs; node kernels, residual cell, saved activations and every
 *   epilogue stay fp32.
 *   matgcn_backward, mode 3: every transposed mix on the graph-mix kernels - the chain's two per step and layer (split by
 *   support slot), the 64-channel x columns of the last step and of the layers, layer 0's narrow x columns when they fill
 *   whole 64-column tiles - runs on k_mix_bf16x3<2>: one 64 x 128 tile shape for odd and even batch rows, partial sums
 *   when one part's reduction is longer than 1 024 indices (the fp32 transposed mix has none).  Its A operand is the plain
 *   stack (the transposed supports) as three bf16 planes that matgcn_forward_train writes into the train buffer on its
 *   side stream, SLOT BY SLOT: [piece][slot][Np rounded up to 32][N rounded up to 64], zero-filled - Np is a multiple of
 *   16, the kernel's K-tile holds 32 reduction indices, and the last tile of a slot must not run into the next slot's
 *   rows.  Layer-0 x columns that take the generic GEMM, every parameter-gradient product, the adjacency gradient and
 *   everything in memory stay fp32.  gcn_off models have no graph mixes: the mode is a no-op there.
 * Buffers: while mode 3 is the effective mode matgcn_workspace_bytes counts the forward's planes (as
 * matgcn_set_mix_precision(3)) and matgcn_train_bytes the plain stack's - 6 bytes per element of [Ks][Np up to 32][N up
 * to 64], behind everything else the mode uses and in front of the deterministic slabs; a mode-3 forward_train or
 * backward on a buffer sized without them returns MATGCN_ERR_SMALL_BUFFER (ask again and re-allocate).  fp32 and modes 1
 * and 2 pay nothing and keep their bits.
 * matgcn_set_deterministic is independent and composes: the mixes meet nothing in memory (the slot parts are added by
 * their consumers), so a deterministic mode-3 backward is bit-reproducible and both matgcn_set_wavefront schedules give
 * the same bits.
 * Measured at Baltimore 403 / B = 64 (MI355X, tools/train_step.py [--bf16x3], one box and one session, the parent build
 * and this one alternating twice, median of 30 steps each): training step 20.11 / 20.02 ms against
 * 21.68 / 21.65 ms in fp32 (-7.4 %), forward_train 6.82 / 6.79 against 7.63 / 7.61 ms, backward 13.11 / 13.10 against
 * 13.91 / 13.89 ms; the parent's fp32 step 21.80 / 21.62 ms - the default path is as fast as before the switch existed.
 * 3 354 624 bytes of planes in the train buffer, 3 194 880 in the workspace.  The per-launch time of k_mix_bf16x3<2>
 * against k_mix_n32<false> under a kernel trace has NOT been measured yet; the backward's 0.8 ms are the only evidence
 * that the transposed three-piece mix is the faster one. */
int matgcn_set_train_bf16x3(int enabled);

/* ---- deterministic backward --------------------------------------------------------------------------------------
 * matgcn_set_deterministic(1): every sum of matgcn_backward that several workgroups (or waves) form together is added
 * in a fixed order, so the gradients (d_h0 included) are bit-identical from run to run for the same inputs, buffers
 * and library settings - matgcn_set_wavefront(0) and (1) included: they give the same bits.  Returns the previous
 * setting; 0 (default) = fp32 atomics, today's kernels and speed; any non-zero value = on.  Governs matgcn_backward
 * only and is read when matgcn_backward is called; independent of both precision settings (training precision modes
 * 0, 1, 2 change operands, not reductions).
 * How each site is ordered:
 *   slabs - each contributor stores its partial sum with plain stores into a slab of its own, indexed by its position
 *   in the grid, and ONE kernel (k_ordered_reduce) adds the slabs in ascending index into the destination: the split
 *   GEMMs (residual nn.Linear weights with their bias rows, head weight, adjacency fallback, pools -> embedding), the
 *   adjacency-gradient tile kernels (at most 16 slices), the pool -> embedding product (a slab per wave), the embedding
 *   gradient (a slab per stack entry) and its stack gains, the narrow residual weight blocks and the column sums (at
 *   most 256 workgroups), the head-fusion gains, the blend scalars (a float per workgroup and step, one reduction per
 *   layer behind its chain);
 *   one contributor - the node weight-gradient kernels (dWp, dBias, the narrow row streams) and the per-node column
 *   sums run one workgroup per node over all steps, so nothing meets in memory;
 *   stream order - launches that accumulate one after the other (time steps, layers, beta = 1 GEMMs) were ordered
 *   already; the accumulations that cross the library's streams (dT and node_emb over the layers) are tied by events
 *   in both schedules, in the same layer order.  Layer 0's fused two-channel residual kernel is replaced by its two
 *   separate kernels, which both schedules then share.
 * Scratch: the slabs live in the caller's `train` buffer, behind everything else the call's mode uses.
 * matgcn_train_bytes counts them while the setting is on; a deterministic matgcn_backward on a buffer sized without
 * them returns MATGCN_ERR_SMALL_BUFFER (ask again and re-allocate).  Size, in floats, each term rounded up to 64:
 *   2 * A + L * T * W,   W = max(ceil(B/64) * N, ceil(B*Np/64), 512) workgroups of a chain kernel,
 *   A = max(16 N^2, 256*128*max(C0,64) + 256*128, 16*hT*CH*64, 32*E*N*d, E*N*d + 64*E*ceil(N*d/256),
 *           256*192*max(C0,16), 256*256, 8*ceil(T*N*od/256)),   E = stack entries + 4
 * - one arena A per stream that runs reductions (the chains' and the weight gradients'), shared by all sites of that
 * stream and all layers: a site's slabs are reduced, in stream order, before the next site writes.  Nothing is
 * allocated by the library.  Measured at Baltimore 403 / B = 64 (MI355X, tools/train_step.py --deterministic, DESIGN.md
 * section 5c): 20 887 040 bytes of slabs; backward 14.3 ms against 13.8 (+3.6 %), training step 22.0 ms against 21.7
 * (+1.7 %); the default path as fast as before the switch existed.  No single site dominates the added time. */
int matgcn_set_deterministic(int enabled);

/* ---- ensemble training: CRPS over dropout samples, backward through the head -----------------------------------------------
 * Dropout sits only in front of end_conv, so the encoder - its saved activations and its backward chain - does not depend
 * on the mask: a step that trains on S samples runs the encoder ONCE in both directions and only the head S times.
 *
 * matgcn_forward_train_mc: matgcn_forward_train with drop_mask = NULL - its kernels, its precision mode, the same bits in
 * `train` and the workspace - with the head replaced by k_head_mc over `samples` masks of the top layer's sequence, sample s
 * drawn at dropout->offset + s.  samples_out (samples, B, out, N, od) is required; mean / std (B, out, N, od) may be NULL.
 * samples_out[s] is bit-equal to what matgcn_forward_mc writes for the same descriptor (fp32 modes) and to
 * matgcn_output_head on seq * mask_s.  Limits as matgcn_forward_mc: in_steps > 24 without fnn_off or out_channels > 64 is
 * MATGCN_ERR_UNSUPPORTED, samples outside 1 .. MATGCN_MAX_MC_SAMPLES is MATGCN_ERR_BAD_ARG; p = 0 is a valid descriptor.
 * `train` must hold matgcn_train_mc_bytes(dims, samples) bytes (less: MATGCN_ERR_SMALL_BUFFER): matgcn_train_bytes of any
 * setting, plus a tail for this pair - two (B, out, N, od) tensors, the partial slabs of the head's weight gradient (at most
 * 256 x out_channels x headT x 64 floats) and samples x out_channels doubles.  matgcn_train_bytes and
 * matgcn_workspace_bytes are unchanged.
 *
 * matgcn_backward_mc: matgcn_backward behind matgcn_forward_train_mc.  d_samples (samples, B, out, N, od) is the gradient
 * w.r.t. samples_out; by linearity every gradient equals the sum over s of what matgcn_backward returns with
 * drop_mask = mask(seed, offset + s) and d_out = d_samples[s] on the same saved activations.  Only the head stage differs
 * (bwd_head_mc beside bwd_head; fp32 in every training precision mode); the chains, the weight-gradient streams, the error
 * exits and the mode that follows the forward are matgcn_backward's.  No mask and no (S, B, T, N, 64) tensor exists:
 *   k_head_mc_dseq   one workgroup per (b, 32-node tile); the 24 x 32 x 64 tile of the sequence gradient stays in 192
 *                    accumulator registers per lane over all samples, d_s . W on the fp32 MFMA, the multiplier drawn at the
 *                    element's position and applied as the product lands; every element is stored once;
 *   k_head_mc_wgrad  32 channels x 12 steps per workgroup, accumulators in registers over its (b, tile) items and all
 *                    samples, one partial slab per workgroup column, added in ascending order by k_ordered_reduce - no
 *                    atomics: the head's gradients have the same bits from run to run in both settings of
 *                    matgcn_set_deterministic (which governs everything behind the head as before);
 *   k_head_mc_dbias_* the bias gradient in two ordered stages, fp64 partial sums.
 * Measured at Baltimore 403 / B = 64 / out = 24 (MI355X, tools/crps_train_time.py bm403 30 3, one process, routes
 * alternating three times, median of 30 steps): the whole step on S = 8 / 32 samples 22.8 / 28.5 ms
 * against 21.0 ms for the seeded masked-MAE step and 166 / 662 ms for S seeded steps; matgcn_forward_train_mc 9.47 ms at
 * S = 32 against matgcn_forward_train 6.95 ms.  Kernels at S = 32 under a kernel trace of the serial schedule: k_head_mc
 * 2.45 ms, k_head_mc_dseq 2.51 ms, k_head_mc_wgrad 1.74 ms - against 0.39 ms each for their 60.8 GFLOP at the nominal fp32
 * MFMA rate: 4.5x to 6.4x off, not near the matrix pipe's time; k_crps_partial + k_loss_final + k_crps_grad 0.159 + 0.016 +
 * 0.162 ms against about 0.04 ms for one read plus one write of the 79 MB of samples.
 *
 * matgcn_crps_loss / matgcn_crps_loss_grad: the CRPS matgcn_mc_scores reports, as a differentiable objective of the samples.
 * Labels, mask, de-scaling and geometry are exactly matgcn_mc_scores' (the series label rule included).  Per unmasked
 * element, in fp64 from the fp32 values, i 0-based in ascending order:
 *   c = (1/S) sum_s |p_s - l| - (1/S^2) sum_i (2i - S + 1) p_(i)
 * result[0] = float32(sum c / M) over all horizons, result[1 + k] horizon k alone; a group that keeps nothing gives 0
 * (matgcn_loss's rule for its masked kinds).  out_steps <= 64.  Gradient of result[0]:
 *   d_samples[s] = upstream * (std / M) * ( sgn(p_s - l) / S - (2 r_s - S + 1) / S^2 ),
 * r_s the 0-based rank of sample s sorted by (value, sample index) - the index decides ties, so the sub-gradient is a
 * definite number -, sgn(0) = 0 as in matgcn_loss's MAE gradient; formed in fp64, rounded once; masked elements get 0 in all
 * S samples.  d_samples MAY be `samples` itself: a workgroup reads its tile completely before it writes it.  The sort is
 * matgcn_mc_scores' LDS bitonic network with its tile rule (64 / 32 / 16 elements by S), over (value, index) pairs in the
 * gradient (96 KB of LDS at most); the padding to a power of two never reaches a result.  Two stages in a fixed order -
 * one workgroup per (b, horizon) row walks the row's tiles, then matgcn_loss's second stage -, no atomics, nothing
 * allocated, all work on the caller's stream.  scratch: caller-owned device memory of matgcn_crps_loss_bytes (=
 * matgcn_loss_bytes) bytes; the gradient call takes the scratch its value call left.  Every argument is checked on the host
 * before anything is launched, with the refusals of matgcn_mc_scores. */
int matgcn_train_mc_bytes(const matgcn_dims* dims, int samples, size_t* bytes);
int matgcn_forward_train_mc(const matgcn_dims* dims, const matgcn_params* params, const void* prepared, const float* X,
                            const matgcn_series* src, const float* h0, const matgcn_dropout* dropout, int samples,
                            float* mean, float* std, float* samples_out, void* workspace, size_t workspace_bytes,
                            void* train, size_t train_bytes, void* stream);
int matgcn_backward_mc(const matgcn_dims* dims, const matgcn_params* params, const void* prepared, const float* X,
                       const matgcn_series* src, const float* h0, const matgcn_dropout* dropout, int samples,
                       const float* d_samples, const matgcn_grads* grads, float* d_h0, void* workspace,
                       size_t workspace_bytes, void* train, size_t train_bytes, void* stream);
int matgcn_crps_loss_bytes(int batch, int out_steps, size_t* bytes);
int matgcn_crps_loss(const float* samples /* (S, B, out, N, od) */, int n_samples, const float* y, const int32_t* label_start, int batch,
                     int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean, float std,
                     float null_val, float min_s, void* scratch, size_t scratch_bytes, float* result /* 1 + out_steps */,
                     void* stream);
int matgcn_crps_loss_grad(const float* samples /* (S, B, out, N, od) */, int n_samples, const float* y, const int32_t* label_start, int batch,
                          int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean,
                          float std, float null_val, float min_s, const void* scratch, size_t scratch_bytes,
                          float upstream, float* d_samples /* (S, B, out, N, od); may alias samples */, void* stream);

/* ---- measurement hooks (bench.py; not on the hot path) ---------------------------------------
 * Time individual kernel launches in situ with HIP events recorded on the caller's stream.
 * enable() creates 2*max_launches events (the only allocation in the library, outside any forward)
 * and selects which kernels are bracketed (bit mask of MATGCN_PROF_*); while enabled every selected
 * launch records an event pair until max_launches is reached.  collect() synchronises the recorded
 * events and writes per-launch milliseconds and kernel kinds; disable() destroys the events. */
enum { MATGCN_PROF_MIX = 1,      /* k_mix<1>: the recurrent step's graph mix (the roofline kernel) */
       MATGCN_PROF_GATE = 2, MATGCN_PROF_UPDATE = 4, MATGCN_PROF_RES = 8, MATGCN_PROF_PX = 16,
       MATGCN_PROF_HEAD = 32,
       MATGCN_PROF_MIX_PRE = 64, /* k_mix<0>: pre-pass mixes (layer-0 fold, x-part chunks) */
       MATGCN_PROF_ALL = 127 };
int matgcn_profile_enable(int kind_mask, int max_launches);
int matgcn_profile_collect(float* ms, int* kinds, int capacity, int* count);
int matgcn_profile_disable(void);

#ifdef __cplusplus
}
#endif
#endif /* MATGCN_H */

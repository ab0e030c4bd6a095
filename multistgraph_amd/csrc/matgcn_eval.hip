// matgcn_eval.hip - host side of everything that evaluates a forecast: training objectives, metric sums, Monte-Carlo
// scores, conformal calibration, region totals and the region loss, and the optimizer step (include/matgcn.h).  Included
// by matgcn_capi.hip inside its extern "C" block, after the kernel files.

namespace {
// The label contract of include/matgcn.h: which y_steps a call may bring.  LABELS_STRICT: y_steps >= out_steps, windows
// or series.  LABELS_SERIES: y_steps >= 1 and y_feat >= 1, and y_steps >= out_steps for windows only.
enum LabelRule { LABELS_STRICT, LABELS_SERIES };
// the one check of (batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, label_start); fills the kernels' view
int label_view(LabelRule rule, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes, int out_dim,
               int y_steps, int y_feat, int y_start, LabelView* v) {
  if (batch < 1 || out_steps < 1 || nodes < 1 || out_dim < 1) return MATGCN_ERR_BAD_ARG;
  if (y_steps < out_steps && (rule == LABELS_STRICT || !label_start)) return MATGCN_ERR_BAD_ARG;
  if (rule == LABELS_SERIES && (y_steps < 1 || y_feat < 1)) return MATGCN_ERR_BAD_ARG;
  if (y_start < 0 || (long)y_start + out_dim > y_feat) return MATGCN_ERR_BAD_ARG;
  v->y = y; v->labelStart = label_start;
  v->outSteps = out_steps; v->N = nodes; v->od = out_dim; v->ySteps = y_steps; v->yFeat = y_feat; v->yStart = y_start;
  return MATGCN_OK;
}
// the affines and the clamp of the descriptor; a lone mean or std is refused
int node_scale(const matgcn_metric_scale* scale, NodeScale* sc) {
  if (!scale) return MATGCN_ERR_NULL;
  if ((scale->mean == nullptr) != (scale->std == nullptr) || (scale->mean2 == nullptr) != (scale->std2 == nullptr))
    return MATGCN_ERR_BAD_ARG;
  sc->mean = scale->mean; sc->std = scale->std; sc->mean2 = scale->mean2; sc->std2 = scale->std2;
  sc->perNode = scale->per_node; sc->clampMin = scale->clamp_min;
  return MATGCN_OK;
}
}  // namespace

int matgcn_masked_mae(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                      int out_dim, int y_steps, int y_feat, int y_start, float mean, float std, float null_val,
                      float min_s, float* partials, float* result, void* stream) {
  if (!pred || !y || !partials || !result) return MATGCN_ERR_NULL;
  LabelView v;      // checked here; k_mae_* keep the reference's parameter list
  RETURN_IF(label_view(LABELS_STRICT, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, &v));
  if (out_steps > 64) return MATGCN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mae_partial, dim3((unsigned)(batch * out_steps)), dim3(256), 0, s, pred, y, label_start, out_steps,
                     nodes, out_dim, y_steps, y_feat, y_start, mean, std, null_val, min_s, partials);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_mae_final, dim3(1), dim3(64), 0, s, partials, batch, out_steps, result);
  return launch_ok();
}

int matgcn_masked_mae_grad(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps,
                           int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean, float std,
                           float null_val, float min_s, const float* partials, const float* upstream, float* d_pred,
                           void* stream) {
  if (!pred || !y || !partials || !upstream || !d_pred) return MATGCN_ERR_NULL;
  LabelView v;
  RETURN_IF(label_view(LABELS_STRICT, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, &v));
  if (out_steps > 64) return MATGCN_ERR_BAD_ARG;
  const size_t total = (size_t)batch * out_steps * nodes * out_dim;
  hipLaunchKernelGGL(k_mae_grad, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, pred, y, label_start,
                     out_steps, nodes, out_dim, y_steps, y_feat, y_start, mean, std, null_val, min_s,
                     partials + 2 * (size_t)batch * out_steps, upstream, total, d_pred);
  return launch_ok();
}

// ---- the executor's training objectives (matgcn_loss.hip) ---------------------------------------------------------------
namespace {
// every check of an objective on (pred, labels); fills its argument block
int loss_check(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
               int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc, size_t scratch_bytes,
               LossArgs* a) {
  size_t need = 0;
  RETURN_IF(matgcn_loss_bytes(batch, out_steps, &need));
  RETURN_IF(label_view(LABELS_STRICT, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, &a->lab));
  if (desc->kind < MATGCN_LOSS_MAE || desc->kind > MATGCN_LOSS_QUANTILE) return MATGCN_ERR_BAD_ARG;
  const float dl = desc->delta;
  if (!(dl - dl == 0.f)) return MATGCN_ERR_BAD_ARG;                                  // inf and NaN
  if (desc->kind == MATGCN_LOSS_QUANTILE && !(dl > 0.f && dl < 1.f)) return MATGCN_ERR_BAD_ARG;
  if (desc->kind == MATGCN_LOSS_HUBER && !(dl > 0.f)) return MATGCN_ERR_BAD_ARG;
  if ((long)nodes * out_dim >= (1L << 31)) return MATGCN_ERR_UNSUPPORTED;
  if (((long)batch * out_steps * nodes * out_dim + 255) / 256 >= (1L << 31)) return MATGCN_ERR_UNSUPPORTED;
  if (scratch_bytes < need) return MATGCN_ERR_SMALL_BUFFER;
  a->pred = pred;
  a->mean = desc->mean; a->std = desc->std; a->nullVal = desc->null_val; a->minS = desc->min_s; a->delta = dl;
  return MATGCN_OK;
}
}  // namespace

// the kernels of kind K: the first four kinds are the masked ones
#define LOSS_KIND_SWITCH(kind, WHAT)                       \
  switch (kind) {                                          \
    case MATGCN_LOSS_MAE: WHAT(MATGCN_LOSS_MAE, 1) break;           \
    case MATGCN_LOSS_MSE: WHAT(MATGCN_LOSS_MSE, 1) break;           \
    case MATGCN_LOSS_RMSE: WHAT(MATGCN_LOSS_RMSE, 1) break;         \
    case MATGCN_LOSS_MAPE: WHAT(MATGCN_LOSS_MAPE, 1) break;         \
    case MATGCN_LOSS_LOGCOSH: WHAT(MATGCN_LOSS_LOGCOSH, 0) break;   \
    case MATGCN_LOSS_HUBER: WHAT(MATGCN_LOSS_HUBER, 0) break;       \
    default: WHAT(MATGCN_LOSS_QUANTILE, 0) break;                   \
  }

int matgcn_loss_bytes(int batch, int out_steps, size_t* bytes) {
  if (!bytes) return MATGCN_ERR_NULL;
  if (batch < 1 || out_steps < 1 || out_steps > 64) return MATGCN_ERR_BAD_ARG;
  if ((long)batch * out_steps >= (1L << 31)) return MATGCN_ERR_UNSUPPORTED;
  *bytes = (2 * (size_t)batch * out_steps + 2) * sizeof(double);
  return MATGCN_OK;
}

namespace {
// the two stages of a checked objective
int loss_launch(const LossArgs& a, int kind, int batch, double* sc, float* result, hipStream_t s) {
  const int out_steps = a.lab.outSteps;
  const dim3 slabs((unsigned)(batch * out_steps));
#define LOSS_PARTIAL(K, M) hipLaunchKernelGGL((k_loss_partial<K, M>), slabs, dim3(LOSS_THREADS), 0, s, a, sc);
  LOSS_KIND_SWITCH(kind, LOSS_PARTIAL)
#undef LOSS_PARTIAL
  CHECK_LAUNCH();
#define LOSS_FINAL(K, M) hipLaunchKernelGGL((k_loss_final<K>), dim3(1), dim3(64), 0, s, sc, batch, out_steps, result);
  LOSS_KIND_SWITCH(kind, LOSS_FINAL)
#undef LOSS_FINAL
  return launch_ok();
}
}  // namespace

int matgcn_loss(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc, void* scratch,
                size_t scratch_bytes, float* result, void* stream) {
  if (!pred || !y || !desc || !scratch || !result) return MATGCN_ERR_NULL;
  LossArgs a;
  RETURN_IF(loss_check(pred, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, desc,
                       scratch_bytes, &a));
  return loss_launch(a, desc->kind, batch, (double*)scratch, result, (hipStream_t)stream);
}

int matgcn_loss_grad(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                     int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc, const void* scratch,
                     size_t scratch_bytes, const float* upstream, float* d_pred, void* stream) {
  if (!pred || !y || !desc || !scratch || !upstream || !d_pred) return MATGCN_ERR_NULL;
  LossArgs a;
  RETURN_IF(loss_check(pred, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, desc,
                       scratch_bytes, &a));
  const size_t total = (size_t)batch * out_steps * nodes * out_dim;
  const double* kept = (const double*)scratch + 2 * (size_t)batch * out_steps;
#define LOSS_GRAD(K, M)                                                                                          \
  hipLaunchKernelGGL((k_loss_grad<K, M>), dim3(blocks_for(total)), dim3(LOSS_THREADS), 0, (hipStream_t)stream, a, kept, \
                     upstream, total, d_pred);
  LOSS_KIND_SWITCH(desc->kind, LOSS_GRAD)
#undef LOSS_GRAD
  return launch_ok();
}

namespace {
// the labels, checked under the strict rule, and the descriptor, checked, into the loose fields MetricArgs keeps
int metric_args(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                int out_dim, int y_steps, int y_feat, int y_start, const matgcn_metric_scale* scale, MetricArgs* a) {
  LabelView v;
  NodeScale sc;
  RETURN_IF(label_view(LABELS_STRICT, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, &v));
  RETURN_IF(node_scale(scale, &sc));
  a->pred = pred; a->y = v.y; a->labelStart = v.labelStart;
  a->mean = sc.mean; a->std = sc.std; a->mean2 = sc.mean2; a->std2 = sc.std2; a->perNode = sc.perNode;
  a->clampMin = sc.clampMin; a->truthMin = scale->truth_min; a->minS = scale->min_s;
  a->outSteps = v.outSteps; a->N = v.N; a->od = v.od; a->ySteps = v.ySteps; a->yFeat = v.yFeat; a->yStart = v.yStart;
  return MATGCN_OK;
}
}  // namespace

int matgcn_metric_sums(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                       int out_dim, int y_steps, int y_feat, int y_start, const matgcn_metric_scale* scale,
                       double* partials, double* sums, int accumulate, void* stream) {
  if (!pred || !y || !scale || !partials || !sums) return MATGCN_ERR_NULL;
  MetricArgs a;
  RETURN_IF(metric_args(pred, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, scale, &a));
  if (out_steps > 64) return MATGCN_ERR_BAD_ARG;
  a.partials = partials;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_metric_partial, dim3((unsigned)(batch * out_steps)), dim3(256), 0, s, a);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_metric_accumulate, dim3((unsigned)out_steps), dim3(64), 0, s, partials, batch, out_steps,
                     accumulate, sums);
  return launch_ok();
}

int matgcn_metric_table(const double* sums, int out_steps, int swap_r2, double* table, void* stream) {
  if (!sums || !table) return MATGCN_ERR_NULL;
  if (out_steps < 1 || out_steps > 64) return MATGCN_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_metric_table, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, out_steps, swap_r2, table);
  return launch_ok();
}

int matgcn_metric_sums_nodes_bytes(int batch, int out_steps, int nodes, int out_dim, size_t* bytes) {
  if (!bytes) return MATGCN_ERR_NULL;
  if (batch < 1 || out_steps < 1 || out_steps > 64 || nodes < 1 || out_dim < 1) return MATGCN_ERR_BAD_ARG;
  if ((long)nodes * out_steps >= (1L << 31)) return MATGCN_ERR_UNSUPPORTED;
  *bytes = 0;      // a thread owns a (horizon, node) and walks the batch itself: no stage-1 partials
  return MATGCN_OK;
}

int matgcn_metric_sums_nodes(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps,
                             int nodes, int out_dim, int y_steps, int y_feat, int y_start,
                             const matgcn_metric_scale* scale, void* scratch, size_t scratch_bytes, double* sums,
                             int accumulate, void* stream) {
  if (!pred || !y || !scale || !sums) return MATGCN_ERR_NULL;
  size_t need = 0;
  RETURN_IF(matgcn_metric_sums_nodes_bytes(batch, out_steps, nodes, out_dim, &need));
  MetricArgs a;
  RETURN_IF(metric_args(pred, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, scale, &a));
  if (need > 0 && !scratch) return MATGCN_ERR_NULL;
  if (scratch_bytes < need) return MATGCN_ERR_SMALL_BUFFER;
  a.partials = nullptr;
  const unsigned blocks = (unsigned)(((long)out_steps * nodes + 63) / 64);
  hipLaunchKernelGGL(k_metric_nodes, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, batch, accumulate, sums);
  return launch_ok();
}

int matgcn_metric_table_rows(const double* sums, int rows, int fold, int swap_r2, double* table, void* stream) {
  if (!sums || !table) return MATGCN_ERR_NULL;
  if (rows < 1 || fold < 1) return MATGCN_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_metric_table_rows, dim3((unsigned)(((long)rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sums,
                     rows, fold, swap_r2, table);
  return launch_ok();
}

// ---- quantiles and probabilistic scores of a Monte-Carlo-dropout ensemble (matgcn_mc_scores.hip) -----------------------
namespace {
// the tile of S samples: P = S rounded up to a power of two, TE = 2^logTE elements with P * TE <= MC_TILE_FLOATS
struct McTile { int P, logTE, ldsBytes; };
McTile mc_tile(int S) {
  McTile t;
  t.P = 1;
  while (t.P < S) t.P <<= 1;
  t.logTE = 6;
  while ((t.P << t.logTE) > MC_TILE_FLOATS) --t.logTE;
  const int bytes = (t.P << t.logTE) * (int)sizeof(float);
  t.ldsBytes = bytes > MC_REDUCE_BYTES ? bytes : MC_REDUCE_BYTES;
  return t;
}
// levels in [0, 1], ascending (NaN fails every comparison) -> the interpolation indices and weights of each
int mc_levels(const float* probs, int n_probs, int S, McLevels* lv) {
  if (n_probs < 1 || n_probs > MATGCN_MAX_MC_QUANTILES) return MATGCN_ERR_BAD_ARG;
  memset(lv, 0, sizeof(*lv));
  lv->n = n_probs;
  for (int k = 0; k < n_probs; ++k) {
    const float q = probs[k];
    if (!(q >= 0.f && q <= 1.f) || (k > 0 && !(q >= probs[k - 1]))) return MATGCN_ERR_BAD_ARG;
    const double h = (double)q * (double)(S - 1);
    int j = (int)floor(h);
    if (j > S - 1) j = S - 1;
    lv->lo[k] = j;
    lv->hi[k] = j + 1 < S ? j + 1 : S - 1;
    lv->g[k] = (float)(h - (double)j);
    lv->q[k] = (double)q;
  }
  const double alpha = 1.0 - ((double)probs[n_probs - 1] - (double)probs[0]);
  lv->winkler = alpha != 0.0 ? 2.0 / alpha : 0.0;
  return MATGCN_OK;
}
// geometry of a score call -> tiles per (b, horizon) row and the number of workgroups
int mc_score_grid(int batch, int out_steps, int nodes, int out_dim, int n_samples, int* tilesPerRow, long* blocks) {
  if (batch < 1 || out_steps < 1 || nodes < 1 || out_dim < 1) return MATGCN_ERR_BAD_ARG;
  if (n_samples < 1 || n_samples > MATGCN_MAX_MC_SAMPLES) return MATGCN_ERR_BAD_ARG;
  const long rowLen = (long)nodes * out_dim;
  if (rowLen >= (1L << 31)) return MATGCN_ERR_UNSUPPORTED;
  const McTile t = mc_tile(n_samples);
  const long tiles = (rowLen + (1L << t.logTE) - 1) >> t.logTE;
  if ((long)batch * out_steps > (1L << 31) / tiles) return MATGCN_ERR_UNSUPPORTED;
  *tilesPerRow = (int)tiles;
  *blocks = (long)batch * out_steps * tiles;
  return MATGCN_OK;
}
// what the three score entry points share: grid, labels (the series rule), levels and tile -> the kernels' view
struct McLaunch { McLevels lv; unsigned blocks; size_t ldsBytes; };
int mc_tile_view(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch, int out_steps,
                 int nodes, int out_dim, int y_steps, int y_feat, int y_start, const float* probs, int n_probs,
                 McTileView* v, McLaunch* l) {
  long blocks = 0;
  RETURN_IF(mc_score_grid(batch, out_steps, nodes, out_dim, n_samples, &v->tilesPerRow, &blocks));
  RETURN_IF(label_view(LABELS_SERIES, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, &v->lab));
  RETURN_IF(mc_levels(probs, n_probs, n_samples, &l->lv));
  const McTile t = mc_tile(n_samples);
  v->samples = samples; v->S = n_samples; v->P = t.P; v->logTE = t.logTE;
  v->E = (long long)batch * out_steps * nodes * out_dim;
  l->blocks = (unsigned)blocks; l->ldsBytes = (size_t)t.ldsBytes;
  return MATGCN_OK;
}
}  // namespace

int matgcn_mc_quantiles(const float* samples, int n_samples, int64_t elems, const float* probs, int n_probs, float mean,
                        float std, float* quantiles, void* stream) {
  if (!samples || !probs || !quantiles) return MATGCN_ERR_NULL;
  if (n_samples < 1 || n_samples > MATGCN_MAX_MC_SAMPLES || elems < 1) return MATGCN_ERR_BAD_ARG;
  McLevels lv;
  RETURN_IF(mc_levels(probs, n_probs, n_samples, &lv));
  const McTile t = mc_tile(n_samples);
  const int64_t blocks = (elems + (1 << t.logTE) - 1) >> t.logTE;
  if (blocks >= (1LL << 31)) return MATGCN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_mc_quantiles, dim3((unsigned)blocks), dim3(256), (size_t)t.ldsBytes, (hipStream_t)stream, samples,
                     lv, n_samples, t.P, t.logTE, (long long)elems, mean, std, quantiles);
  return launch_ok();
}

int matgcn_mc_scores_bytes(int batch, int out_steps, int nodes, int out_dim, int n_samples, int n_probs, size_t* bytes) {
  if (!bytes) return MATGCN_ERR_NULL;
  if (n_probs < 1 || n_probs > MATGCN_MAX_MC_QUANTILES) return MATGCN_ERR_BAD_ARG;
  int tilesPerRow = 0;
  long blocks = 0;
  RETURN_IF(mc_score_grid(batch, out_steps, nodes, out_dim, n_samples, &tilesPerRow, &blocks));
  *bytes = (size_t)blocks * (MATGCN_MC_SCORE_SUMS + n_probs) * sizeof(double);
  return MATGCN_OK;
}

int matgcn_mc_scores(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch,
                     int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean, float std,
                     float null_val, float min_s, const float* probs, int n_probs, void* scratch, size_t scratch_bytes,
                     double* sums, int accumulate, void* stream) {
  if (!samples || !y || !probs || !scratch || !sums) return MATGCN_ERR_NULL;
  McScoreArgs a;
  McTileView t;
  McLaunch l;
  RETURN_IF(mc_tile_view(samples, n_samples, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start,
                         probs, n_probs, &t, &l));
  mc_loose_fields(t, &a);
  const int K = MATGCN_MC_SCORE_SUMS + n_probs;
  if (scratch_bytes < (size_t)l.blocks * K * sizeof(double)) return MATGCN_ERR_SMALL_BUFFER;
  a.mean = mean; a.std = std; a.nullVal = null_val; a.minS = min_s;
  a.partials = (double*)scratch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mc_scores, dim3(l.blocks), dim3(256), l.ldsBytes, s, a, l.lv);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_mc_accumulate, dim3((unsigned)out_steps), dim3(64), 0, s, a.partials, batch, out_steps,
                     a.tilesPerRow, K, accumulate, sums);
  return launch_ok();
}

int matgcn_mc_quantiles_scaled(const float* samples, int n_samples, int64_t elems, int nodes, int out_dim,
                               const float* probs, int n_probs, const matgcn_metric_scale* scale, float* quantiles,
                               void* stream) {
  if (!samples || !probs || !quantiles) return MATGCN_ERR_NULL;
  NodeScale sc;
  RETURN_IF(node_scale(scale, &sc));
  if (n_samples < 1 || n_samples > MATGCN_MAX_MC_SAMPLES || elems < 1 || nodes < 1 || out_dim < 1)
    return MATGCN_ERR_BAD_ARG;
  const long rowLen = (long)nodes * out_dim;
  if (rowLen >= (1L << 31)) return MATGCN_ERR_UNSUPPORTED;
  if (elems % rowLen != 0) return MATGCN_ERR_BAD_ARG;
  McLevels lv;
  RETURN_IF(mc_levels(probs, n_probs, n_samples, &lv));
  const McTile t = mc_tile(n_samples);
  const int64_t blocks = (elems + (1 << t.logTE) - 1) >> t.logTE;
  if (blocks >= (1LL << 31)) return MATGCN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_mc_quantiles_scaled, dim3((unsigned)blocks), dim3(256), (size_t)t.ldsBytes, (hipStream_t)stream,
                     samples, lv, n_samples, t.P, t.logTE, (long long)elems, (int)rowLen, out_dim, sc, quantiles);
  return launch_ok();
}

int matgcn_mc_scores_nodes_bytes(int batch, int out_steps, int nodes, int out_dim, int n_samples, int n_probs,
                                 size_t* bytes) {
  if (!bytes) return MATGCN_ERR_NULL;
  if (n_probs < 1 || n_probs > MATGCN_MAX_MC_QUANTILES || out_steps > 64) return MATGCN_ERR_BAD_ARG;
  int tilesPerRow = 0;
  long blocks = 0;
  RETURN_IF(mc_score_grid(batch, out_steps, nodes, out_dim, n_samples, &tilesPerRow, &blocks));
  // one term per element and sum: stage 2 adds them one at a time
  *bytes = (size_t)batch * out_steps * nodes * out_dim * (MATGCN_MC_SCORE_SUMS + n_probs) * sizeof(double);
  return MATGCN_OK;
}

int matgcn_mc_scores_nodes(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch,
                           int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start,
                           const matgcn_metric_scale* scale, float null_val, const float* probs, int n_probs,
                           void* scratch, size_t scratch_bytes, double* sums, int accumulate, void* stream) {
  if (!samples || !y || !probs || !scratch || !sums) return MATGCN_ERR_NULL;
  McNodeArgs a;
  McLaunch l;
  RETURN_IF(node_scale(scale, &a.sc));
  if (out_steps > 64) return MATGCN_ERR_BAD_ARG;
  RETURN_IF(mc_tile_view(samples, n_samples, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start,
                         probs, n_probs, &a.t, &l));
  const int K = MATGCN_MC_SCORE_SUMS + n_probs;
  if (scratch_bytes < (size_t)a.t.E * K * sizeof(double)) return MATGCN_ERR_SMALL_BUFFER;
  a.truthMin = scale->truth_min; a.minS = scale->min_s; a.nullVal = null_val;
  double* terms = (double*)scratch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mc_scores_nodes, dim3(l.blocks), dim3(256), l.ldsBytes, s, a, l.lv, terms);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_mc_accumulate_nodes, dim3(blocks_for((size_t)out_steps * nodes * K)), dim3(256), 0, s, terms, batch,
                     out_steps, nodes, out_dim, K, accumulate, sums);
  return launch_ok();
}

// ---- the ensemble's CRPS as a training objective (matgcn_crps.hip) ---------------------------------------------------------
int matgcn_crps_loss_bytes(int batch, int out_steps, size_t* bytes) { return matgcn_loss_bytes(batch, out_steps, bytes); }

namespace {
// every check of the two CRPS entry points - the refusals of matgcn_mc_scores (grid, samples, the series label rule), the
// scratch of matgcn_loss -; fills the kernels' argument block and the tile
int crps_check(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch, int out_steps,
               int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean, float std, float null_val,
               float min_s, size_t scratch_bytes, CrpsArgs* a, long* blocks) {
  RETURN_IF(mc_score_grid(batch, out_steps, nodes, out_dim, n_samples, &a->tilesPerRow, blocks));
  RETURN_IF(label_view(LABELS_SERIES, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, &a->lab));
  size_t need = 0;
  RETURN_IF(matgcn_crps_loss_bytes(batch, out_steps, &need));
  if (scratch_bytes < need) return MATGCN_ERR_SMALL_BUFFER;
  const McTile t = mc_tile(n_samples);
  a->samples = samples; a->S = n_samples; a->P = t.P; a->logTE = t.logTE;
  a->E = (long long)batch * out_steps * nodes * out_dim;
  a->mean = mean; a->std = std; a->nullVal = null_val; a->minS = min_s;
  return MATGCN_OK;
}
}  // namespace

int matgcn_crps_loss(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch,
                     int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean, float std,
                     float null_val, float min_s, void* scratch, size_t scratch_bytes, float* result, void* stream) {
  if (!samples || !y || !scratch || !result) return MATGCN_ERR_NULL;
  CrpsArgs a;
  long blocks = 0;
  RETURN_IF(crps_check(samples, n_samples, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, mean,
                       std, null_val, min_s, scratch_bytes, &a, &blocks));
  hipStream_t s = (hipStream_t)stream;
  double* sc = (double*)scratch;
  hipLaunchKernelGGL(k_crps_partial, dim3((unsigned)(batch * out_steps)), dim3(256), (size_t)mc_tile(n_samples).ldsBytes, s,
                     a, sc);
  CHECK_LAUNCH();
  // the second stage of matgcn_loss's masked kinds: sum / count per horizon and over all, 0 where nothing is kept, and the
  // count behind the slabs for the gradient
  hipLaunchKernelGGL((k_loss_final<MATGCN_LOSS_MAE>), dim3(1), dim3(64), 0, s, sc, batch, out_steps, result);
  return launch_ok();
}

int matgcn_crps_loss_grad(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch,
                          int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start, float mean,
                          float std, float null_val, float min_s, const void* scratch, size_t scratch_bytes,
                          float upstream, float* d_samples, void* stream) {
  if (!samples || !y || !scratch || !d_samples) return MATGCN_ERR_NULL;
  CrpsArgs a;
  long blocks = 0;
  RETURN_IF(crps_check(samples, n_samples, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, mean,
                       std, null_val, min_s, scratch_bytes, &a, &blocks));
  // (value, sample index) pairs: the floats of the tile and one 16-bit index each - 96 KB at most, opted into once
  const int lds = (a.P << a.logTE) * (int)(sizeof(float) + sizeof(unsigned short));
  if (lds > 64 * 1024) {
    int& ready = dev_current().crpsLds;
    if (!ready) {
      RETURN_IF(lds_opt_in(reinterpret_cast<const void*>(k_crps_grad), MC_TILE_FLOATS * 6));
      ready = 1;
    }
  }
  const double* kept = (const double*)scratch + 2 * (size_t)batch * out_steps;
  hipLaunchKernelGGL(k_crps_grad, dim3((unsigned)blocks), dim3(256), (size_t)lds, (hipStream_t)stream, a, kept, upstream,
                     d_samples);
  return launch_ok();
}

// ---- split conformal calibration of the band (matgcn_conformal.hip) -------------------------------------------------------
int matgcn_mc_conformity(const float* samples, int n_samples, const float* y, const int32_t* label_start, int batch,
                         int out_steps, int nodes, int out_dim, int y_steps, int y_feat, int y_start,
                         const matgcn_metric_scale* scale, float null_val, const float* probs, int n_probs, float* scores,
                         void* stream) {
  if (!samples || !y || !probs || !scores) return MATGCN_ERR_NULL;
  McConformityArgs a;
  McTileView t;
  McLaunch l;
  RETURN_IF(node_scale(scale, &a.sc));
  if (out_steps > 64 || n_probs < 2) return MATGCN_ERR_BAD_ARG;
  RETURN_IF(mc_tile_view(samples, n_samples, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start,
                         probs, n_probs, &t, &l));
  const McLevels& all = l.lv;
  McLevels lv;
  // the kernel reads the outer two levels only
  memset(&lv, 0, sizeof(lv));
  lv.n = 2;
  const int src[2] = {0, n_probs - 1};
  for (int k = 0; k < 2; ++k) {
    lv.lo[k] = all.lo[src[k]]; lv.hi[k] = all.hi[src[k]]; lv.g[k] = all.g[src[k]]; lv.q[k] = all.q[src[k]];
  }
  lv.winkler = all.winkler;
  mc_loose_fields(t, &a);
  a.truthMin = scale->truth_min; a.minS = scale->min_s; a.nullVal = null_val; a.scores = scores;
  hipLaunchKernelGGL(k_mc_conformity, dim3(l.blocks), dim3(256), l.ldsBytes, (hipStream_t)stream, a, lv);
  return launch_ok();
}

namespace {
// the store (rows, out_steps, cols) of the two calibration entry points: counts >= 1, out_steps in 1 .. 64, the element
// count inside int64; what a 32-bit index or count of the kernels cannot hold is MATGCN_ERR_UNSUPPORTED
int conf_store(int64_t rows, int out_steps, int cols, int grouping) {
  if (rows < 1 || out_steps < 1 || out_steps > 64 || cols < 1 || (grouping != 0 && grouping != 1)) return MATGCN_ERR_BAD_ARG;
  const int64_t rowElems = (int64_t)out_steps * cols;                 // < 2^37
  if (rows > INT64_MAX / rowElems) return MATGCN_ERR_BAD_ARG;
  const int64_t walk = grouping ? rows : rows * (int64_t)cols;        // what one group's count and row index run over
  if (rows > INT32_MAX || walk > (int64_t)INT32_MAX - 4 * CONF_ROW_THREADS) return MATGCN_ERR_UNSUPPORTED;
  return MATGCN_OK;
}
}  // namespace

int matgcn_conformal_quantile(const float* scores, int64_t rows, int out_steps, int cols, int grouping, double coverage,
                              float* margin, int32_t* count, void* stream) {
  if (!scores || !margin || !count) return MATGCN_ERR_NULL;
  RETURN_IF(conf_store(rows, out_steps, cols, grouping));
  if (!(coverage > 0.0 && coverage <= 1.0)) return MATGCN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (grouping)
    hipLaunchKernelGGL(k_conformal_select_cols, dim3((unsigned)((cols + CONF_COLS - 1) / CONF_COLS), (unsigned)out_steps),
                       dim3(256), 0, s, scores, (int)rows, out_steps, cols, coverage, margin, count);
  else
    hipLaunchKernelGGL(k_conformal_select_rows, dim3((unsigned)out_steps), dim3(CONF_ROW_THREADS), 0, s, scores, (int)rows,
                       out_steps, cols, coverage, margin, count);
  return launch_ok();
}

int matgcn_conformal_coverage(const float* scores, int64_t rows, int out_steps, int cols, int grouping, const float* margin,
                              int64_t* counts, int accumulate, void* stream) {
  if (!scores || !margin || !counts) return MATGCN_ERR_NULL;
  RETURN_IF(conf_store(rows, out_steps, cols, grouping));
  hipStream_t s = (hipStream_t)stream;
  if (grouping)
    hipLaunchKernelGGL(k_conformal_coverage_cols, dim3(blocks_for((size_t)out_steps * cols)), dim3(256), 0, s, scores,
                       (int)rows, out_steps, cols, margin, accumulate, (long long*)counts);
  else
    hipLaunchKernelGGL(k_conformal_coverage_rows, dim3((unsigned)out_steps), dim3(256), 0, s, scores, (int)rows, out_steps,
                       cols, margin, accumulate, (long long*)counts);
  return launch_ok();
}

// ---- totals over groups of nodes (matgcn_regions.hip) ----------------------------------------------------------------------
namespace {
// the map: non-null host and device offsets, G >= 1, members >= 0 (node may be null without members), ptr[0] = 0,
// non-decreasing, ptr[G] = members
int group_map(const matgcn_groups* groups, GroupMap* m) {
  if (!groups) return MATGCN_ERR_NULL;
  if (!groups->ptr || !groups->ptr_dev) return MATGCN_ERR_NULL;
  if (groups->n_groups < 1 || groups->n_members < 0) return MATGCN_ERR_BAD_ARG;
  if (groups->n_members > 0 && !groups->node) return MATGCN_ERR_NULL;
  if (groups->ptr[0] != 0 || groups->ptr[groups->n_groups] != groups->n_members) return MATGCN_ERR_BAD_ARG;
  for (int g = 0; g < groups->n_groups; ++g)
    if (groups->ptr[g + 1] < groups->ptr[g]) return MATGCN_ERR_BAD_ARG;
  m->ptr = groups->ptr_dev; m->node = groups->node; m->weight = groups->weight; m->G = groups->n_groups;
  return MATGCN_OK;
}
// (rows, nodes, out_dim) in and (rows, G, out_dim) out: counts >= 1, both element counts inside int64, a row and the
// chains of a tile inside a 32-bit index
int group_shape(int64_t rows, int nodes, int out_dim, int n_groups) {
  if (rows < 1 || nodes < 1 || out_dim < 1) return MATGCN_ERR_BAD_ARG;
  const int64_t rowLen = (int64_t)nodes * out_dim, outLen = (int64_t)n_groups * out_dim;   // < 2^62
  if (rows > INT64_MAX / rowLen || rows > INT64_MAX / outLen) return MATGCN_ERR_BAD_ARG;
  if (rowLen > INT32_MAX || outLen > INT32_MAX / GROUP_MAX_ROWS) return MATGCN_ERR_UNSUPPORTED;
  return MATGCN_OK;
}
int group_walk(GroupWalkArgs& a, int64_t rows, hipStream_t s) {
  a.total = (long long)rows * a.map.G * a.od;
  const long long blocks = (a.total + GROUP_THREADS - 1) / GROUP_THREADS;
  if (blocks > INT32_MAX) return MATGCN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_group_walk, dim3((unsigned)blocks), dim3(GROUP_THREADS), 0, s, a);
  return launch_ok();
}
}  // namespace

int matgcn_group_sums(const float* values, int64_t rows, int nodes, int out_dim, const matgcn_metric_scale* scale,
                      const matgcn_groups* groups, float* out, void* stream) {
  if (!values || !out) return MATGCN_ERR_NULL;
  NodeScale sc;
  RETURN_IF(node_scale(scale, &sc));
  GroupMap map;
  RETURN_IF(group_map(groups, &map));
  RETURN_IF(group_shape(rows, nodes, out_dim, map.G));
  const int rowLen = nodes * out_dim, stride = rowLen | 1;
  hipStream_t s = (hipStream_t)stream;
  if (stride > GROUP_TILE_FLOATS) {      // a row that no tile holds: walk it in global memory
    GroupWalkArgs w;
    memset(&w, 0, sizeof(w));
    w.src = values; w.N = nodes; w.od = out_dim; w.sc = sc; w.map = map; w.out = out;
    return group_walk(w, rows, s);
  }
  // rows per tile: what 32 KB hold (a longer row: that row alone), a multiple of 4 where it can be (a tile then starts
  // 16-byte aligned whenever the tensor does), halved while that leaves fewer than 1024 tiles to spread over the CUs
  int R = stride > GROUP_ROWS_FLOATS ? 1 : GROUP_ROWS_FLOATS / stride;
  // the map goes into LDS behind the rows when it is small (its offsets, and its weights if any)
  const int mapFloats = groups->n_members <= GROUP_MAP_FLOATS ? groups->n_members * (groups->weight ? 2 : 1) : INT32_MAX;
  const bool staged = mapFloats <= GROUP_MAP_FLOATS && R * stride + mapFloats <= GROUP_TILE_FLOATS;
  if (R > GROUP_MAX_ROWS) R = GROUP_MAX_ROWS;
  if (R > 4) R &= ~3;
  while (R > 4 && (rows + R - 1) / R < 1024) R = (R / 2 + 3) & ~3;
  const int64_t tiles = (rows + R - 1) / R;
  if (tiles > INT32_MAX) return MATGCN_ERR_UNSUPPORTED;
  GroupTileArgs a;
  a.values = values; a.rows = rows; a.N = nodes; a.od = out_dim; a.rowLen = rowLen; a.stride = stride; a.R = R;
  a.mapAt = staged ? R * stride : -1; a.members = groups->n_members;
  a.stepQuot = 4 * GROUP_THREADS / rowLen; a.stepRem = 4 * GROUP_THREADS % rowLen;
  a.sc = sc; a.map = map; a.out = out;
  const size_t ldsFloats = (size_t)R * stride + (staged ? mapFloats : 0);       // <= GROUP_TILE_FLOATS
  hipLaunchKernelGGL(k_group_sums_tile, dim3((unsigned)tiles), dim3(GROUP_THREADS), ldsFloats * sizeof(float), s, a);
  return launch_ok();
}

int matgcn_group_label_sums(const float* y, const int32_t* label_start, int batch, int out_steps, int nodes, int out_dim,
                            int y_steps, int y_feat, int y_start, const matgcn_metric_scale* scale,
                            const matgcn_groups* groups, float* out, void* stream) {
  if (!y || !out) return MATGCN_ERR_NULL;
  GroupWalkArgs w;
  memset(&w, 0, sizeof(w));
  RETURN_IF(node_scale(scale, &w.sc));
  RETURN_IF(group_map(groups, &w.map));
  if (batch < 1 || out_steps < 1) return MATGCN_ERR_BAD_ARG;
  RETURN_IF(group_shape((int64_t)batch * out_steps, nodes, out_dim, w.map.G));
  LabelView v;
  RETURN_IF(label_view(LABELS_SERIES, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, &v));
  w.src = v.y; w.labelStart = v.labelStart; w.labels = 1;
  w.outSteps = v.outSteps; w.ySteps = v.ySteps; w.yFeat = v.yFeat; w.yStart = v.yStart;
  w.N = v.N; w.od = v.od; w.out = out;
  return group_walk(w, (int64_t)batch * out_steps, (hipStream_t)stream);
}

// ---- a training objective on region totals, value and gradient (matgcn_region_loss.hip) ------------------------------------
namespace {
// the scratch of the pair: the totals of the predictions, the totals of the labels (rows * G * od floats each, together a
// multiple of 8 bytes), matgcn_loss's own scratch for (B, out, G, od), then the descriptor's (mean, std) as two floats,
// which the total kernels read through their scale descriptor
struct RegionScratch {
  float* P; float* L;
  double* loss; size_t lossBytes;
  float* affine;
  size_t bytes;
};
int region_scratch(int batch, int out_steps, int n_groups, int out_dim, void* scratch, RegionScratch* r) {
  size_t lossBytes = 0;
  RETURN_IF(matgcn_loss_bytes(batch, out_steps, &lossBytes));
  if (n_groups < 1 || out_dim < 1) return MATGCN_ERR_BAD_ARG;
  if ((int64_t)n_groups * out_dim > INT32_MAX / GROUP_MAX_ROWS) return MATGCN_ERR_UNSUPPORTED;
  const size_t totals = (size_t)batch * out_steps * n_groups * out_dim;        // < 2^31 * 2^23
  char* at = (char*)scratch;
  r->P = (float*)at; r->L = r->P + totals;
  r->loss = (double*)(at + 2 * totals * sizeof(float)); r->lossBytes = lossBytes;
  r->affine = (float*)(at + 2 * totals * sizeof(float) + lossBytes);
  r->bytes = 2 * totals * sizeof(float) + lossBytes + 2 * sizeof(float);
  return MATGCN_OK;
}
// every check of the pair that does not concern the by-node map; fills the layout, the by-group map and the argument block
// of the objective on the totals: P against L over G nodes, identity affine, the caller's kind, null value, min_s and delta
int region_check(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                 int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc,
                 const matgcn_groups* by_group, const void* scratch, size_t scratch_bytes, RegionScratch* rs, GroupMap* map,
                 LossArgs* onTotals) {
  RETURN_IF(loss_check(pred, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, desc, SIZE_MAX,
                       onTotals));
  RETURN_IF(group_map(by_group, map));
  RETURN_IF(group_shape((int64_t)batch * out_steps, nodes, out_dim, map->G));
  RETURN_IF(region_scratch(batch, out_steps, map->G, out_dim, const_cast<void*>(scratch), rs));
  matgcn_loss_desc identity = *desc;
  identity.mean = 0.f; identity.std = 1.f;
  RETURN_IF(loss_check(rs->P, rs->L, nullptr, batch, out_steps, map->G, out_dim, out_steps, out_dim, 0, &identity, SIZE_MAX,
                       onTotals));
  if (scratch_bytes < rs->bytes) return MATGCN_ERR_SMALL_BUFFER;
  if ((reinterpret_cast<uintptr_t>(scratch) & 7) != 0) return MATGCN_ERR_BAD_ARG;
  return MATGCN_OK;
}
}  // namespace

int matgcn_region_loss_bytes(int batch, int out_steps, int n_groups, int out_dim, size_t* bytes) {
  if (!bytes) return MATGCN_ERR_NULL;
  RegionScratch rs;
  RETURN_IF(region_scratch(batch, out_steps, n_groups, out_dim, nullptr, &rs));
  *bytes = rs.bytes;
  return MATGCN_OK;
}

int matgcn_region_loss(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps, int nodes,
                       int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc,
                       const matgcn_groups* by_group, void* scratch, size_t scratch_bytes, float* result, void* stream) {
  if (!pred || !y || !desc || !by_group || !scratch || !result) return MATGCN_ERR_NULL;
  RegionScratch rs;
  GroupMap map;
  LossArgs onTotals;
  RETURN_IF(region_check(pred, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, desc, by_group,
                         scratch, scratch_bytes, &rs, &map, &onTotals));
  hipLaunchKernelGGL(k_region_affine, dim3(1), dim3(64), 0, (hipStream_t)stream, rs.affine, desc->mean, desc->std);
  CHECK_LAUNCH();
  matgcn_metric_scale scale;
  memset(&scale, 0, sizeof(scale));
  scale.mean = rs.affine; scale.std = rs.affine + 1;
  scale.clamp_min = scale.truth_min = __builtin_nanf(""); scale.min_s = -1.f;
  RETURN_IF(matgcn_group_sums(pred, (int64_t)batch * out_steps, nodes, out_dim, &scale, by_group, rs.P, stream));
  RETURN_IF(matgcn_group_label_sums(y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, &scale,
                                    by_group, rs.L, stream));
  // matgcn_loss's two launches on the block region_check had loss_check fill: not through the entry point, no second check
  return loss_launch(onTotals, desc->kind, batch, rs.loss, result, (hipStream_t)stream);
}

int matgcn_region_loss_grad(const float* pred, const float* y, const int32_t* label_start, int batch, int out_steps,
                            int nodes, int out_dim, int y_steps, int y_feat, int y_start, const matgcn_loss_desc* desc,
                            const matgcn_groups* by_group, const matgcn_groups* by_node, const void* scratch,
                            size_t scratch_bytes, const float* upstream, const float* base, float* d_pred, void* stream) {
  // pred, y and label_start are checked, not read: the totals in scratch are all the gradient reads of them
  if (!pred || !y || !desc || !by_group || !by_node || !scratch || !upstream || !d_pred) return MATGCN_ERR_NULL;
  RegionScratch rs;
  GroupMap map, nodeMap;
  LossArgs onTotals;
  RETURN_IF(region_check(pred, y, label_start, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, desc, by_group,
                         scratch, scratch_bytes, &rs, &map, &onTotals));
  RETURN_IF(group_map(by_node, &nodeMap));
  if (nodeMap.G != nodes || by_node->n_members != by_group->n_members) return MATGCN_ERR_BAD_ARG;
  RegionGradArgs a;
  memset(&a, 0, sizeof(a));
  a.id = onTotals;
  a.kept = rs.loss + 2 * (size_t)batch * out_steps;
  a.upstream = upstream; a.base = base; a.dpred = d_pred;
  a.rows = (long long)batch * out_steps;
  a.N = nodes; a.od = out_dim; a.rowLen = nodes * out_dim;
  a.G = map.G; a.GC = map.G * out_dim;
  a.members = by_node->n_members;
  a.std = desc->std;
  a.nptr = nodeMap.ptr; a.ngroup = nodeMap.node; a.nweight = nodeMap.weight;
  hipStream_t s = (hipStream_t)stream;
  if (a.GC > REGION_Q_FLOATS) {       // no tile holds one row's coefficients: recompute them per membership
    const long long total = a.rows * a.rowLen;
    const long long blocks = (total + REGION_THREADS - 1) / REGION_THREADS;
    if (blocks > INT32_MAX) return MATGCN_ERR_UNSUPPORTED;
#define REGION_WALK(K, M) \
    hipLaunchKernelGGL((k_region_grad_walk<K, M>), dim3((unsigned)blocks), dim3(REGION_THREADS), 0, s, a, total);
    LOSS_KIND_SWITCH(desc->kind, REGION_WALK)
#undef REGION_WALK
    return launch_ok();
  }
  // rows per tile: what the coefficient budget and 16 elements per thread allow, halved while that leaves fewer than
  // REGION_MIN_TILES tiles to spread over the CUs
  int R = REGION_Q_FLOATS / a.GC;
  const int byElems = REGION_TILE_ELEMS / a.rowLen;
  if (R > byElems) R = byElems < 1 ? 1 : byElems;
  if (R > REGION_MAX_ROWS) R = REGION_MAX_ROWS;
  while (R > 1 && (a.rows + R - 1) / R < REGION_MIN_TILES) R = (R + 1) / 2;
  a.R = R;
  const int mapFloats = a.members <= REGION_MAP_FLOATS ? a.members * (a.nweight ? 2 : 1) : INT32_MAX;
  a.staged = mapFloats <= REGION_MAP_FLOATS;
  const long long tiles = (a.rows + R - 1) / R;
  if (tiles > INT32_MAX) return MATGCN_ERR_UNSUPPORTED;
  const size_t ldsFloats = (size_t)R * a.GC + (a.staged ? mapFloats : 0);      // <= REGION_Q_FLOATS + REGION_MAP_FLOATS
#define REGION_TILE(K, M)                                                                                       \
  hipLaunchKernelGGL((k_region_grad_tile<K, M>), dim3((unsigned)tiles), dim3(REGION_THREADS), ldsFloats * sizeof(float), \
                     s, a);
  LOSS_KIND_SWITCH(desc->kind, REGION_TILE)
#undef REGION_TILE
  return launch_ok();
}

// ---- global gradient norm, clip and Adam over a table of tensors (matgcn_optim.hip) --------------------------------------
namespace {
// A float hyperparameter read as the decimal its caller wrote: the shortest one that rounds to the same float (0.999f ->
// 0.999).  Any double inside the float's rounding interval is a legitimate reading of it; this one makes 1 - beta2 the
// 1e-3 torch forms from the Python double, where the float's own value would give 0.99998713e-3 - 1.3e-5 off, a hundred
// fp32 roundings, in every exp_avg_sq.  (The printf family and strtod follow LC_NUMERIC together, so the pair is
// consistent under any locale.)
double opt_decimal(float f) {
  if (!(f == f) || f - f != 0.f) return (double)f;
  char buf[40];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof buf, "%.*g", prec, (double)f);
    const double d = strtod(buf, nullptr);
    if ((float)d == f) return d;
  }
  return (double)f;
}
// checks every tensor; chunks = sum over the tensors of ceil(numel / OPT_CHUNK)
int opt_check_table(const matgcn_opt_tensor* t, int n, bool norm_only, int64_t* chunks) {
  if (!t) return MATGCN_ERR_NULL;
  if (n < 1) return MATGCN_ERR_BAD_ARG;
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (t[i].numel < 0) return MATGCN_ERR_BAD_ARG;
    if (t[i].numel == 0) continue;
    if (!t[i].grad) return MATGCN_ERR_NULL;
    if (!norm_only && (!t[i].param || !t[i].exp_avg || !t[i].exp_avg_sq)) return MATGCN_ERR_NULL;
    total += (t[i].numel + OPT_CHUNK - 1) / OPT_CHUNK;
    if (total >= (1LL << 31)) return MATGCN_ERR_UNSUPPORTED;
  }
  *chunks = total;
  return MATGCN_OK;
}
// the launch table of the tensors first .. first + count - 1; returns its chunks
int opt_fill_table(const matgcn_opt_tensor* t, int first, int count, OptTable* T) {
  memset(T, 0, sizeof(*T));
  T->n = count;
  int chunks = 0;
  for (int i = 0; i < count; ++i) {
    const matgcn_opt_tensor& s = t[first + i];
    T->param[i] = s.param; T->grad[i] = s.grad; T->expAvg[i] = s.exp_avg; T->expAvgSq[i] = s.exp_avg_sq;
    T->numel[i] = s.numel;
    chunks += (int)((s.numel + OPT_CHUNK - 1) / OPT_CHUNK);
    T->chunkEnd[i] = chunks;
  }
  return chunks;
}
}  // namespace

int matgcn_grad_norm_bytes(const matgcn_opt_tensor* t, int n, size_t* bytes) {
  if (!bytes) return MATGCN_ERR_NULL;
  int64_t chunks = 0;
  RETURN_IF(opt_check_table(t, n, true, &chunks));
  *bytes = (size_t)chunks * sizeof(double);
  return MATGCN_OK;
}

int matgcn_grad_norm(const matgcn_opt_tensor* t, int n, void* scratch, size_t scratch_bytes, float* total_norm,
                     void* stream) {
  if (!total_norm) return MATGCN_ERR_NULL;
  int64_t chunks = 0;
  RETURN_IF(opt_check_table(t, n, true, &chunks));
  if (chunks > 0 && !scratch) return MATGCN_ERR_NULL;
  if (scratch_bytes < (size_t)chunks * sizeof(double)) return MATGCN_ERR_SMALL_BUFFER;
  hipStream_t s = (hipStream_t)stream;
  int base = 0;
  for (int first = 0; first < n; first += OPT_MAX_TENSORS) {
    OptTable T;
    const int c = opt_fill_table(t, first, n - first < OPT_MAX_TENSORS ? n - first : OPT_MAX_TENSORS, &T);
    if (c == 0) continue;
    hipLaunchKernelGGL(k_opt_sumsq, dim3((unsigned)c), dim3(OPT_THREADS), 0, s, T, base, (double*)scratch);
    CHECK_LAUNCH();
    base += c;
  }
  hipLaunchKernelGGL(k_opt_norm_finish, dim3(1), dim3(OPT_THREADS), 0, s, (const double*)scratch, (int)chunks, total_norm);
  return launch_ok();
}

int matgcn_adam_step(const matgcn_opt_tensor* t, int n, const matgcn_adam* hp, const float* total_norm, void* stream) {
  if (!hp) return MATGCN_ERR_NULL;
  int64_t chunks = 0;
  RETURN_IF(opt_check_table(t, n, false, &chunks));
  if (!(hp->lr >= 0.f) || !(hp->eps >= 0.f) || !(hp->weight_decay >= 0.f)) return MATGCN_ERR_BAD_ARG;   // NaN fails too
  if (!(hp->beta1 >= 0.f && hp->beta1 < 1.f) || !(hp->beta2 >= 0.f && hp->beta2 < 1.f)) return MATGCN_ERR_BAD_ARG;
  if (hp->step < 1 || hp->max_norm != hp->max_norm) return MATGCN_ERR_BAD_ARG;
  if (hp->max_norm > 0.f && !total_norm) return MATGCN_ERR_NULL;
  // the scalars of torch's _single_tensor_adam, formed in double as Python forms them; those of the fp32 part rounded once
  const double b1 = opt_decimal(hp->beta1), b2 = opt_decimal(hp->beta2), step = (double)hp->step;
  const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
  OptScalars h;
  h.w1 = 1.0 - b1;
  h.w2 = 1.0 - b2;
  h.beta2 = b2;
  h.weightDecay = opt_decimal(hp->weight_decay);
  h.stepSize = (float)(opt_decimal(hp->lr) / bc1);
  h.bc2Sqrt = (float)sqrt(bc2);
  h.eps = hp->eps;
  h.maxNorm = hp->max_norm;
  hipStream_t s = (hipStream_t)stream;
  for (int first = 0; first < n; first += OPT_MAX_TENSORS) {
    OptTable T;
    const int c = opt_fill_table(t, first, n - first < OPT_MAX_TENSORS ? n - first : OPT_MAX_TENSORS, &T);
    if (c == 0) continue;
    hipLaunchKernelGGL(k_opt_adam, dim3((unsigned)c), dim3(OPT_THREADS), 0, s, T, h, total_norm);
    CHECK_LAUNCH();
  }
  return MATGCN_OK;
}

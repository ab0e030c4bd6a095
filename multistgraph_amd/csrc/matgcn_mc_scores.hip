// matgcn_mc_scores.hip - empirical quantiles and probabilistic scores of a Monte-Carlo-dropout ensemble
// (matgcn_mc_quantiles / matgcn_mc_scores, and on the re-transformed scale matgcn_mc_quantiles_scaled / per (horizon,
// node) matgcn_mc_scores_nodes; include/matgcn.h).  Included by matgcn_capi.hip.
//
// Input: the sample-major tensor matgcn_forward_mc writes to samples_out, samples (S, E), E = B * out * N * od.
// One sort core serves both entry points: a workgroup of 256 threads takes a tile of TE consecutive elements and all S
// samples of each - every sample row of the tile is read from HBM once, TE consecutive floats at a time -, de-scales
// on load and sorts each element's column in LDS with a bitonic network over P = S rounded up to a power of two.
//   - The rows S .. P-1 are filled with +inf: with finite samples they end up behind the S real values and no result
//     reads them (every index a result uses is <= S-1).  Columns behind the end of the tile's row are filled with 0 and
//     never stored or scored.  A non-finite sample only permutes a column differently (every compare-exchange writes
//     back the two values it read): no index depends on data, so nothing can leave the tile or loop.
//   - LDS layout x[row][e], e fastest: the lanes of a compare-exchange that hold adjacent elements hit adjacent banks.
//     TE = 64 and 32 put a whole 32-lane group on one row (32 banks, conflict-free).  TE = 16 puts two pair indices
//     pr, pr + 1 into a group; their rows i, i' differ in bit 0 - opposite halves of the 32 banks - for every stride
//     j >= 2 but are both even for j = 1 (i = 2 pr), a 2-way conflict in 10 of the 55 stages at S = 1024.  So sample s
//     lives in row s ^ ((s >> 1) & 1), a permutation inside every aligned group of four rows that gives rows 2 pr and
//     2 pr + 2 opposite parity and leaves i, i + 1 (i even) opposite as well: conflict-free for every stride.
//   - The tile is P * TE <= 16 384 floats (64 KB): TE = 64 up to S = 256, 32 up to 512, 16 up to 1024 (mc_tile_log2,
//     chosen on the host) - two workgroups fit into the 160 KB of a CU, and no kernel needs the opt-in above 64 KB.
// Nothing is allocated, no atomics (series_row counts a violated range contract, as everywhere), no result depends on
// the order the workgroups run in: the scores are one partial per workgroup in caller-owned scratch and a second kernel
// that adds them in ascending index (k_mc_accumulate, as k_metric_accumulate).
//
// Arithmetic whose bits the header promises is written through scale_affine (matgcn_kernels.hip) and the helpers below,
// with contraction switched off: hipcc fuses a * b + c by default (the __fmul_rn / __fadd_rn of the HIP headers are plain
// operators and fuse as well), which would make the bits depend on the compiler.

constexpr int MC_MAX_PROBS = 8;
constexpr int MC_SCORE_SUMS = 5;                         // count, CRPS, covered, width, Winkler (+ one pinball sum per level)
constexpr int MC_MAX_SUMS = MC_SCORE_SUMS + MC_MAX_PROBS;
constexpr int MC_TILE_FLOATS = 16384;
constexpr int MC_REDUCE_BYTES = 256 * 2 * (int)sizeof(double);   // k_mc_scores: two fp64 partial sums per thread

// lo + g * (hi - lo) as three roundings (fp32): numpy's "linear" rule in float32 arithmetic
__device__ __forceinline__ float mc_lerp(float lo, float hi, float g) {
#pragma clang fp contract(off)
  const float d = hi - lo;
  const float t = g * d;
  return lo + t;
}
// a + c * m as two roundings (fp64)
__device__ __forceinline__ double mc_axpy(double a, double c, double m) {
#pragma clang fp contract(off)
  const double t = c * m;
  return a + t;
}
__device__ __forceinline__ double mc_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

struct McLevels {
  int n;                       // levels (1 .. MC_MAX_PROBS)
  int lo[MC_MAX_PROBS];        // j = floor(h), h = (double)q * (S - 1)
  int hi[MC_MAX_PROBS];        // min(j + 1, S - 1)
  float g[MC_MAX_PROBS];       // (float)(h - j)
  double q[MC_MAX_PROBS];      // (double)q
  double winkler;              // 2 / alpha, alpha = 1 - (q_last - q_first) in double; 0 for alpha = 0
};

__device__ __forceinline__ int mc_row(int s) { return s ^ ((s >> 1) & 1); }

// Sorts every column of the loaded tile ascending (bitonic network over the P rows).  Called by all 256 threads; begins
// and ends with a barrier.
__device__ __forceinline__ void mc_sort_network(float* __restrict__ x, int P, int logTE) {
  const int TE = 1 << logTE, tid = threadIdx.x;
  __syncthreads();
  const int pairs = (P >> 1) << logTE;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = tid; idx < pairs; idx += 256) {
        const int pr = idx >> logTE, e = idx & (TE - 1);
        const int i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), l = i | j;   // i < l < P
        float* pa = x + (mc_row(i) << logTE) + e;
        float* pb = x + (mc_row(l) << logTE) + e;
        const float a = *pa, b = *pb;
        const bool swap = (a > b) == ((i & k) == 0);
        *pa = swap ? b : a;
        *pb = swap ? a : b;
      }
      __syncthreads();
    }
  }
}

// Loads the tile (columns e0 .. e0 + nValid - 1 of `samples`, all S rows), de-scaled, and sorts every column ascending.
// Called by all 256 threads; ends with a barrier.
__device__ __forceinline__ void mc_sort_tile(float* __restrict__ x, const float* __restrict__ samples, int S, int P,
                                             int logTE, size_t E, size_t e0, int nValid, float mean, float std) {
  const int TE = 1 << logTE, tid = threadIdx.x;
  for (int idx = tid; idx < (P << logTE); idx += 256) {
    const int s = idx >> logTE, e = idx & (TE - 1);
    float v = __builtin_inff();
    if (e >= nValid) v = 0.f;
    else if (s < S) v = scale_affine(samples[(size_t)s * E + e0 + e], std, mean);
    x[(mc_row(s) << logTE) + e] = v;
  }
  mc_sort_network(x, P, logTE);
}

// mc_sort_tile with the descriptor of the node-grouped entry points (NodeScale) in place of the two scalars.  256 is a
// multiple of TE, so a thread loads one column e = tid & (TE - 1) only: `node` is that column's node (read where
// e < nValid only) and its affines are fetched once.
__device__ __forceinline__ void mc_sort_tile_scaled(float* __restrict__ x, const float* __restrict__ samples, int S, int P,
                                                    int logTE, size_t E, size_t e0, int nValid, int node,
                                                    const NodeScale& sc) {
  const int TE = 1 << logTE, tid = threadIdx.x, e = tid & (TE - 1);
  const bool live = e < nValid, clamp = sc.clampMin == sc.clampMin;
  float sd = 1.f, mu = 0.f, sd2 = 1.f, mu2 = 0.f;
  if (live && sc.std) { sd = sc.std[sc.perNode ? node : 0]; mu = sc.mean[sc.perNode ? node : 0]; }
  if (live && sc.std2) { sd2 = sc.std2[node]; mu2 = sc.mean2[node]; }
  for (int s = tid >> logTE; s < P; s += 256 >> logTE) {
    float v = __builtin_inff();
    if (!live) v = 0.f;
    else if (s < S) {
      v = samples[(size_t)s * E + e0 + e];
      if (sc.std) v = scale_affine(v, sd, mu);
      if (sc.std2) v = scale_affine(v, sd2, mu2);
      if (clamp && v < sc.clampMin) v = sc.clampMin;
    }
    x[(mc_row(s) << logTE) + e] = v;
  }
  mc_sort_network(x, P, logTE);
}

__device__ __forceinline__ float mc_quantile(const float* x, int logTE, int e, const McLevels& lv, int k) {
  return mc_lerp(x[(mc_row(lv.lo[k]) << logTE) + e], x[(mc_row(lv.hi[k]) << logTE) + e], lv.g[k]);
}

// quantiles (n_probs, E): one workgroup per tile of TE consecutive elements
__global__ __launch_bounds__(256) void k_mc_quantiles(const float* __restrict__ samples, McLevels lv, int S, int P,
                                                      int logTE, long long E, float mean, float std,
                                                      float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float mcTile[];
  const int TE = 1 << logTE;
  const size_t e0 = (size_t)blockIdx.x << logTE;
  const long long left = E - (long long)e0;
  const int nValid = left < TE ? (int)left : TE;
  mc_sort_tile(mcTile, samples, S, P, logTE, (size_t)E, e0, nValid, mean, std);
  for (int idx = threadIdx.x; idx < (lv.n << logTE); idx += 256) {
    const int k = idx >> logTE, e = idx & (TE - 1);
    if (e < nValid) out[(size_t)k * E + e0 + e] = mc_quantile(mcTile, logTE, e, lv, k);
  }
}

// k_mc_quantiles with the descriptor: element g of the (.., N, od) tensor belongs to node (g / od) % N
__global__ __launch_bounds__(256) void k_mc_quantiles_scaled(const float* __restrict__ samples, McLevels lv, int S, int P,
                                                             int logTE, long long E, int rowLen, int od, NodeScale sc,
                                                             float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float mcTile[];
  const int TE = 1 << logTE;
  const size_t e0 = (size_t)blockIdx.x << logTE;
  const long long left = E - (long long)e0;
  const int nValid = left < TE ? (int)left : TE;
  const int node = (int)((e0 + (threadIdx.x & (TE - 1))) % (size_t)rowLen) / od;
  mc_sort_tile_scaled(mcTile, samples, S, P, logTE, (size_t)E, e0, nValid, node, sc);
  for (int idx = threadIdx.x; idx < (lv.n << logTE); idx += 256) {
    const int k = idx >> logTE, e = idx & (TE - 1);
    if (e < nValid) out[(size_t)k * E + e0 + e] = mc_quantile(mcTile, logTE, e, lv, k);
  }
}

// What the three score kernels share: the samples and labels of a call and its tiling, one workgroup per tile of TE
// consecutive elements of one (b, horizon) row of N * od
struct McTileView {
  const float* samples;   // (S, B, out, N, od)
  LabelView lab;
  int S, P, logTE;
  int tilesPerRow;
  long long E;
};
// the tile of this workgroup: its row (b, o), its first position r0 in the row and first element e0, its valid columns
struct McTileAt { int b, o, r0, nValid; size_t e0; };
__device__ __forceinline__ McTileAt mc_tile_at(const McTileView& t) {
  const int rowLen = t.lab.N * t.lab.od;
  const int row = blockIdx.x / t.tilesPerRow, tile = blockIdx.x - row * t.tilesPerRow;
  McTileAt at;
  at.b = row / t.lab.outSteps; at.o = row - at.b * t.lab.outSteps;
  at.r0 = tile << t.logTE;
  at.nValid = min(1 << t.logTE, rowLen - at.r0);
  at.e0 = (size_t)row * rowLen + at.r0;
  return at;
}

// host: the view, field by field, into a block that keeps its own argument order (McScoreArgs, McConformityArgs)
template <class Args>
void mc_loose_fields(const McTileView& t, Args* a) {
  a->samples = t.samples; a->y = t.lab.y; a->labelStart = t.lab.labelStart;
  a->S = t.S; a->P = t.P; a->logTE = t.logTE; a->tilesPerRow = t.tilesPerRow; a->E = t.E;
  a->outSteps = t.lab.outSteps; a->N = t.lab.N; a->od = t.lab.od;
  a->ySteps = t.lab.ySteps; a->yFeat = t.lab.yFeat; a->yStart = t.lab.yStart;
}

// k_mc_scores keeps the argument order and every statement it had before LabelView and McTileView: with the view embedded
// it measured slower than that by more than the run-to-run gap in one session of three, and its
// instructions move with any rewording (sharing statements with k_mc_scores_nodes once cost it 18 scalar spills)
struct McScoreArgs {
  const float* samples;   // (S, B, out, N, od)
  const float* y;         // the fields of LabelView
  const int* labelStart;
  int S, P, logTE;
  int outSteps, N, od, ySteps, yFeat, yStart, tilesPerRow;
  long long E;
  float mean, std, nullVal, minS;
  double* partials;       // [B * out * tilesPerRow][5 + n]
};

// stage 1: one workgroup per tile of one (b, horizon) row of N * od elements -> partials[block][5 + n]
__global__ __launch_bounds__(256) void k_mc_scores(McScoreArgs a, McLevels lv) {
  extern __shared__ __attribute__((aligned(16))) float mcTile[];
  const int logTE = a.logTE, TE = 1 << logTE, tid = threadIdx.x;
  const int rowLen = a.N * a.od;
  const int row = blockIdx.x / a.tilesPerRow, t = blockIdx.x - row * a.tilesPerRow;
  const int b = row / a.outSteps, o = row - b * a.outSteps;
  const int r0 = t << logTE;
  const int nValid = min(TE, rowLen - r0);
  const size_t e0 = (size_t)row * rowLen + r0;
  mc_sort_tile(mcTile, a.samples, a.S, a.P, logTE, (size_t)a.E, e0, nValid, a.mean, a.std);

  // thread (slot, e): the samples i = slot, slot + slots, .. of element e
  const int e = tid & (TE - 1), slot = tid >> logTE, slots = 256 >> logTE;
  const bool inRow = e < nValid;
  float l = 0.f;
  if (inRow) {
    // label_row and label_at written out: through them the compiler schedules this kernel differently (see above)
    const size_t yrow = a.labelStart ? series_row((long)a.labelStart[b] + o, a.ySteps) : (size_t)b * a.ySteps + o;
    const int r = r0 + e, n = r / a.od, c = r - n * a.od;
    l = scale_affine(a.y[(yrow * a.N + n) * a.yFeat + a.yStart + c], a.std, a.mean);
    if (fabsf(l) < a.minS) l = 0.f;
  }
  const bool nanMask = a.nullVal != a.nullVal;
  const bool keep = inRow && (nanMask ? l == l : l != a.nullVal);
  const double ld = (double)l;
  double sAbs = 0.0, sWgt = 0.0;
  for (int i = slot; i < a.S; i += slots) {
    const double xi = (double)mcTile[(mc_row(i) << logTE) + e];
    sAbs += fabs(xi - ld);
    sWgt += mc_mul((double)(2 * i - a.S + 1), xi);      // exact: an integer below 2^11 times an fp32 value
  }
  float qv[MC_MAX_PROBS];
#pragma unroll
  for (int k = 0; k < MC_MAX_PROBS; ++k) qv[k] = (slot == 0 && k < lv.n) ? mc_quantile(mcTile, logTE, e, lv, k) : 0.f;
  __syncthreads();                                      // the sorted tile has been read: its floats become the scratch
  double* red = reinterpret_cast<double*>(mcTile);
  red[2 * tid] = sAbs; red[2 * tid + 1] = sWgt;
  __syncthreads();
  if (tid >= 64) return;                                // wave 0 holds slot 0 of every element (TE <= 64)
  double v[MC_MAX_SUMS];
#pragma unroll
  for (int k = 0; k < MC_MAX_SUMS; ++k) v[k] = 0.0;
  if (tid < TE && keep) {
    double A = 0.0, W = 0.0;
    for (int s = 0; s < slots; ++s) { A += red[2 * ((s << logTE) + e)]; W += red[2 * ((s << logTE) + e) + 1]; }
    const double Sd = (double)a.S;
    float qFirst = 0.f, qLast = 0.f;
#pragma unroll
    for (int k = 0; k < MC_MAX_PROBS; ++k) {
      if (k == 0) qFirst = qv[k];
      if (k == lv.n - 1) qLast = qv[k];
    }
    const double width = (double)qLast - (double)qFirst;
    v[0] = 1.0;
    v[1] = A / Sd - W / (Sd * Sd);
    v[2] = (qFirst <= l && l <= qLast) ? 1.0 : 0.0;
    v[3] = width;
    v[4] = mc_axpy(mc_axpy(width, lv.winkler, fmax((double)qFirst - ld, 0.0)), lv.winkler, fmax(ld - (double)qLast, 0.0));
#pragma unroll
    for (int k = 0; k < MC_MAX_PROBS; ++k) {
      if (k < lv.n) {
        const double d = ld - (double)qv[k];
        v[MC_SCORE_SUMS + k] = fmax(mc_mul(lv.q[k], d), mc_mul(lv.q[k] - 1.0, d));
      }
    }
  }
  const int K = MC_SCORE_SUMS + lv.n;
#pragma unroll
  for (int k = 0; k < MC_MAX_SUMS; ++k) {
    double s = v[k];
    for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_down(s, sh, 64);
    if (tid == 0 && k < K) a.partials[(size_t)blockIdx.x * K + k] = s;
  }
}

// stage 2: block o, thread k: sums[o][k] (+)= the partials of horizon o in ascending (b, tile) order
__global__ __launch_bounds__(64) void k_mc_accumulate(const double* __restrict__ partials, int B, int outSteps,
                                                      int tilesPerRow, int K, int accumulate, double* __restrict__ sums) {
  const int o = blockIdx.x, k = threadIdx.x;
  if (k >= K) return;
  double v = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* p = partials + ((size_t)b * outSteps + o) * tilesPerRow * K + k;
    for (int t = 0; t < tilesPerRow; ++t) v += p[(size_t)t * K];
  }
  sums[o * K + k] = (accumulate ? sums[o * K + k] : 0.0) + v;
}

// ---- the same scores grouped per (horizon, node) (matgcn_mc_scores_nodes) ------------------------------------------------
// A tile of consecutive elements of a (b, horizon) row spans several nodes, and with od > 1 a node's channels can sit in
// two tiles, so stage 1 keeps k_mc_scores' grid - one sort per tile, every sample read once - and hands the 5 + n terms
// of every element (zeros for a masked one) to stage 2, which owns one (horizon, node, sum) per thread and adds its
// terms one at a time in ascending (b, c) onto the stored value: a chain of adds whose order the data alone fixes.
struct McNodeArgs {
  McTileView t;
  NodeScale sc;
  float truthMin, minS, nullVal;
};
// the label of element (n, c) of the tile's row on the re-transformed scale, filtered; false where a mask drops it
__device__ __forceinline__ bool mc_node_label(const McNodeArgs& a, const McTileAt& at, int n, int c, float& l) {
  l = descale_node(a.sc, n, label_at(a.t.lab, label_row(a.t.lab, at.b, at.o), n, c));
  const bool keep = !(a.truthMin == a.truthMin) || l > a.truthMin;
  if (fabsf(l) < a.minS) l = 0.f;
  return keep && (a.nullVal != a.nullVal ? l == l : l != a.nullVal);
}

// terms: [E][5 + n]
__global__ __launch_bounds__(256) void k_mc_scores_nodes(McNodeArgs a, McLevels lv, double* __restrict__ terms) {
  extern __shared__ __attribute__((aligned(16))) float mcTile[];
  const McTileView& t = a.t;
  const int logTE = t.logTE, TE = 1 << logTE, tid = threadIdx.x, S = t.S;
  const McTileAt at = mc_tile_at(t);
  const int e = tid & (TE - 1);
  const int r = at.r0 + e, n = r / t.lab.od, c = r - n * t.lab.od;   // a node of the row where e < nValid
  const bool inRow = e < at.nValid;
  mc_sort_tile_scaled(mcTile, t.samples, S, t.P, logTE, (size_t)t.E, at.e0, at.nValid, n, a.sc);

  float l = 0.f;
  bool keep = false;
  if (inRow) keep = mc_node_label(a, at, n, c, l);
  // from here to the terms v[]: the statements of k_mc_scores, which stays as it was (sharing them through inline
  // functions cost that kernel 18 scalar-register spills); tests hold the two kernels' sums together
  const int slot = tid >> logTE, slots = 256 >> logTE;
  const double ld = (double)l;
  double sAbs = 0.0, sWgt = 0.0;
  for (int i = slot; i < S; i += slots) {
    const double xi = (double)mcTile[(mc_row(i) << logTE) + e];
    sAbs += fabs(xi - ld);
    sWgt += mc_mul((double)(2 * i - S + 1), xi);        // exact: an integer below 2^11 times an fp32 value
  }
  float qv[MC_MAX_PROBS];
#pragma unroll
  for (int k = 0; k < MC_MAX_PROBS; ++k) qv[k] = (slot == 0 && k < lv.n) ? mc_quantile(mcTile, logTE, e, lv, k) : 0.f;
  __syncthreads();                                      // the sorted tile has been read: its floats become the scratch
  double* red = reinterpret_cast<double*>(mcTile);
  red[2 * tid] = sAbs; red[2 * tid + 1] = sWgt;
  __syncthreads();
  if (tid >= TE || !inRow) return;                      // slot 0 holds every element of the tile
  double v[MC_MAX_SUMS];
#pragma unroll
  for (int k = 0; k < MC_MAX_SUMS; ++k) v[k] = 0.0;
  if (keep) {
    double A = 0.0, W = 0.0;
    for (int s = 0; s < slots; ++s) { A += red[2 * ((s << logTE) + e)]; W += red[2 * ((s << logTE) + e) + 1]; }
    const double Sd = (double)S;
    float qFirst = 0.f, qLast = 0.f;
#pragma unroll
    for (int k = 0; k < MC_MAX_PROBS; ++k) {
      if (k == 0) qFirst = qv[k];
      if (k == lv.n - 1) qLast = qv[k];
    }
    const double width = (double)qLast - (double)qFirst;
    v[0] = 1.0;
    v[1] = A / Sd - W / (Sd * Sd);
    v[2] = (qFirst <= l && l <= qLast) ? 1.0 : 0.0;
    v[3] = width;
    v[4] = mc_axpy(mc_axpy(width, lv.winkler, fmax((double)qFirst - ld, 0.0)), lv.winkler, fmax(ld - (double)qLast, 0.0));
#pragma unroll
    for (int k = 0; k < MC_MAX_PROBS; ++k) {
      if (k < lv.n) {
        const double d = ld - (double)qv[k];
        v[MC_SCORE_SUMS + k] = fmax(mc_mul(lv.q[k], d), mc_mul(lv.q[k] - 1.0, d));
      }
    }
  }
  const int K = MC_SCORE_SUMS + lv.n;
  double* out = terms + (at.e0 + e) * K;
#pragma unroll
  for (int k = 0; k < MC_MAX_SUMS; ++k)
    if (k < K) out[k] = v[k];
}

// stage 2: thread (o, n, k): sums[o][n][k] = (stored or 0) + the terms of its elements, one add each, ascending (b, c)
__global__ __launch_bounds__(256) void k_mc_accumulate_nodes(const double* __restrict__ terms, int B, int outSteps, int N,
                                                             int od, int K, int accumulate, double* __restrict__ sums) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)outSteps * N * K) return;
  const int k = (int)(idx % K);
  const size_t on = idx / K;
  const int n = (int)(on % N), o = (int)(on / N);
  double v = accumulate ? sums[idx] : 0.0;
  for (int b = 0; b < B; ++b) {
    const double* p = terms + ((((size_t)b * outSteps + o) * N + n) * od) * K + k;
    for (int c = 0; c < od; ++c) v += p[(size_t)c * K];
  }
  sums[idx] = v;
}

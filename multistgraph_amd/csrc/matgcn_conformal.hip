// matgcn_conformal.hip - split conformal calibration of the Monte-Carlo-dropout band (matgcn_mc_conformity,
// matgcn_conformal_quantile, matgcn_conformal_coverage; include/matgcn.h).  Included by matgcn_capi.hip after
// matgcn_mc_scores.hip, whose sort core (mc_sort_tile_scaled, mc_quantile, the tile choice) it uses unchanged.
//
//   - k_mc_conformity: the grid of k_mc_scores_nodes - one workgroup per tile of a (b, horizon) row, every sample row
//     read once - and, per element, the conformalized-quantile-regression score s = max(Q_first - l, l - Q_last); a
//     masked or filtered element stores a quiet NaN, so every element of the output is written.
//   - k_conformal_select_cols / k_conformal_select_rows: the k-th smallest valid score of every group, exactly, by radix
//     select over order-preserving 32-bit keys: four passes of 8 bits, each a 256-bin histogram in LDS built with LDS
//     integer adds, all four inside one launch.  A workgroup owns its groups alone: no global atomics, no scratch, and
//     only integer counts are added, so no result depends on the order anything runs in.  Every loop bound is a
//     host-known count (rows, cols, 256, 4): a NaN, an infinity or a tie changes which bin is counted, never a trip
//     count or an address outside the histogram.
//   - k_conformal_coverage_*: per group the number of valid scores and of those <= the margin, integer sums.
// Nothing beyond row rows - 1 of the store is read.

constexpr int CONF_COLS = 64;                 // grouping 1: columns per workgroup (one histogram each: 64 x 256 bins = 64 KB)
constexpr int CONF_ROW_THREADS = 1024;        // grouping 0: threads of the one workgroup of a horizon
constexpr int CONF_ROW_COPIES = 32;           // grouping 0: copies of the histogram, one per LDS bank (256 x 32 bins = 32 KB)

// a - b as one rounding (fp32); max of two of them: the score
__device__ __forceinline__ float conf_score(float qFirst, float l, float qLast) {
#pragma clang fp contract(off)
  const float below = qFirst - l;
  const float above = l - qLast;
  return fmaxf(below, above);
}

// order-preserving key of a float: ascending keys = ascending values (-0 before +0; NaN never gets here)
__device__ __forceinline__ unsigned conf_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? (u ^ 0xFFFFFFFFu) : (u | 0x80000000u);
}
__device__ __forceinline__ float conf_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : (k ^ 0xFFFFFFFFu));
}
// k = max(1, ceil((double)(n + 1) * coverage)): one fp64 product.  coverage <= 1, so k <= n + 1 fits an int.
__device__ __forceinline__ int conf_rank(int n, double coverage) {
  const double k = ceil(mc_mul((double)n + 1.0, coverage));
  return k < 1.0 ? 1 : (int)k;
}

// k_mc_conformity keeps the argument order it had before LabelView (samples, labels, tile, geometry): with the view
// embedded it measured slower than that by more than the run-to-run gap at S = 32
struct McConformityArgs {
  const float* samples;   // (S, B, out, N, od)
  const float* y;         // the fields of LabelView
  const int* labelStart;
  int S, P, logTE;
  int outSteps, N, od, ySteps, yFeat, yStart, tilesPerRow;
  long long E;
  NodeScale sc;
  float truthMin, minS, nullVal;
  float* scores;          // (B, out, N, od)
};

// lv holds the outer two levels only (n = 2): first at 0, last at 1
__global__ __launch_bounds__(256) void k_mc_conformity(McConformityArgs a, McLevels lv) {
  extern __shared__ __attribute__((aligned(16))) float mcTile[];
  const int logTE = a.logTE, TE = 1 << logTE, tid = threadIdx.x;
  const int rowLen = a.N * a.od;
  const int row = blockIdx.x / a.tilesPerRow, t = blockIdx.x - row * a.tilesPerRow;
  const int b = row / a.outSteps, o = row - b * a.outSteps;
  const int r0 = t << logTE;
  const int nValid = min(TE, rowLen - r0);
  const size_t e0 = (size_t)row * rowLen + r0;
  const int e = tid & (TE - 1);
  const int r = r0 + e, n = r / a.od, c = r - n * a.od;   // a node of the row where e < nValid
  mc_sort_tile_scaled(mcTile, a.samples, a.S, a.P, logTE, (size_t)a.E, e0, nValid, n, a.sc);
  if (tid >= TE || e >= nValid) return;                   // slot 0 holds every element of the tile
  // label, filter and mask: the statements of mc_node_label
  const LabelView v = {a.y, a.labelStart, a.outSteps, a.N, a.od, a.ySteps, a.yFeat, a.yStart};
  float l = descale_node(a.sc, n, label_at(v, label_row(v, b, o), n, c));
  bool keep = !(a.truthMin == a.truthMin) || l > a.truthMin;
  if (fabsf(l) < a.minS) l = 0.f;
  keep = keep && (a.nullVal != a.nullVal ? l == l : l != a.nullVal);
  const float qFirst = mc_quantile(mcTile, logTE, e, lv, 0), qLast = mc_quantile(mcTile, logTE, e, lv, 1);
  a.scores[e0 + e] = keep ? conf_score(qFirst, l, qLast) : __builtin_nanf("");
}

// ---- the margin per (horizon, column): grid (ceil(cols / 64), out), 256 threads = 64 columns x 4 row lanes ---------------
// hist[bin][column]: the 64 lanes of a wave hold 64 different columns, so an LDS add never meets another lane's address
// and lanes c, c + 32 (the two halves an LDS instruction is served in) share a bank.  The histogram fills the 64 KB a
// workgroup gets without an opt-in, so the search state (prefix, rank left) lives in registers: the four row lanes of a
// column each walk its 256 bins and arrive at the same numbers.
__global__ __launch_bounds__(256) void k_conformal_select_cols(const float* __restrict__ scores, int rows, int outSteps,
                                                               int cols, double coverage, float* __restrict__ margin,
                                                               int* __restrict__ count) {
  __shared__ int hist[256 * CONF_COLS];
  const int tid = threadIdx.x, c = tid & (CONF_COLS - 1), lane = tid >> 6;
  const int o = blockIdx.y, col = blockIdx.x * CONF_COLS + c;
  const bool live = col < cols;
  const float* src = scores + (size_t)o * cols + (live ? col : 0);
  const size_t stride = (size_t)outSteps * cols;
  unsigned prefix = 0u;
  int k = 1, nValid = 0;
  bool open = false;                                                  // k > n: the margin is +inf
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 256 * CONF_COLS; i += 256) hist[i] = 0;
    __syncthreads();
    if (live) {
      for (int r = lane; r < rows; r += 4) {
        const float v = src[(size_t)r * stride];
        if (v == v) {
          const unsigned key = conf_key(v);
          if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(((key >> shift) & 255u) << 6) + c], 1);
        }
      }
    }
    __syncthreads();
    if (pass == 0) {
      for (int j = 0; j < 256; ++j) nValid += hist[(j << 6) + c];
      k = conf_rank(nValid, coverage);
      open = k > nValid;
      if (open) k = 1;
    }
    // the bin whose running count first reaches k, and the rank left inside it
    int cum = 0, bin = 255, left = 1;
    bool found = false;
    for (int j = 0; j < 256; ++j) {
      const int h = hist[(j << 6) + c];
      if (!found && cum + h >= k) { found = true; bin = j; left = k - cum; }
      cum += h;
    }
    prefix = (prefix << 8) | (unsigned)bin;
    k = left;
    __syncthreads();                                                  // every lane has read the histogram: the next pass clears it
  }
  if (lane == 0 && live) {
    margin[(size_t)o * cols + col] = open ? __builtin_inff() : conf_unkey(prefix);
    count[(size_t)o * cols + col] = nValid;
  }
}

// ---- the margin per horizon: one workgroup of 1024 threads per horizon walks its rows x cols scores ----------------------
// hist[bin][copy], copy = thread & 31: the lanes of a wave that meet in one bin (ties) add to 32 different banks.
__global__ __launch_bounds__(CONF_ROW_THREADS) void k_conformal_select_rows(const float* __restrict__ scores, int rows,
                                                                            int outSteps, int cols, double coverage,
                                                                            float* __restrict__ margin,
                                                                            int* __restrict__ count) {
  __shared__ int hist[256 * CONF_ROW_COPIES];
  __shared__ int total[256];
  __shared__ unsigned prefixS;
  __shared__ int rankS, nS, openS;
  const int tid = threadIdx.x, copy = tid & (CONF_ROW_COPIES - 1);
  const int o = blockIdx.x;
  const int elems = rows * cols;                                      // < 2^31 (checked on the host)
  const float* src = scores + (size_t)o * cols;
  const size_t stride = (size_t)outSteps * cols;
  if (tid == 0) { prefixS = 0u; rankS = 1; nS = 0; openS = 0; }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 256 * CONF_ROW_COPIES; i += CONF_ROW_THREADS) hist[i] = 0;
    __syncthreads();
    const unsigned want = prefixS;
    for (int i0 = 0; i0 < elems; i0 += 4 * CONF_ROW_THREADS) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * CONF_ROW_THREADS + tid;
        const int ic = i < elems ? i : 0;                             // i < elems + 4096 <= INT_MAX (host check)
        const int r = ic / cols;
        v[u] = i < elems ? src[(size_t)r * stride + (ic - r * cols)] : __builtin_nanf("");
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (v[u] == v[u]) {
          const unsigned key = conf_key(v[u]);
          if (pass == 0 || (key >> (shift + 8)) == want)
            atomicAdd(&hist[(((key >> shift) & 255u) << 5) + copy], 1);
        }
      }
    }
    __syncthreads();
    if (tid < 256) {
      int sum = 0;
      for (int j = 0; j < CONF_ROW_COPIES; ++j) sum += hist[(tid << 5) + ((j + tid) & (CONF_ROW_COPIES - 1))];
      total[tid] = sum;
    }
    __syncthreads();
    if (tid == 0) {
      int k = rankS;
      if (pass == 0) {
        int n = 0;
        for (int j = 0; j < 256; ++j) n += total[j];
        k = conf_rank(n, coverage);
        nS = n;
        openS = k > n;
        if (k > n) k = 1;
      }
      int cum = 0, bin = 255, left = 1;
      bool found = false;
      for (int j = 0; j < 256; ++j) {
        const int h = total[j];
        if (!found && cum + h >= k) { found = true; bin = j; left = k - cum; }
        cum += h;
      }
      prefixS = (want << 8) | (unsigned)bin;
      rankS = left;
    }
    __syncthreads();
  }
  if (tid == 0) {
    margin[o] = openS ? __builtin_inff() : conf_unkey(prefixS);
    count[o] = nS;
  }
}

// ---- coverage counts: counts[g] = (stored or 0) + {valid scores, valid scores <= margin[g]} ------------------------------
// per (horizon, column): one thread per group walks the rows (adjacent threads, adjacent columns)
__global__ __launch_bounds__(256) void k_conformal_coverage_cols(const float* __restrict__ scores, int rows, int outSteps,
                                                                 int cols, const float* __restrict__ margin, int accumulate,
                                                                 long long* __restrict__ counts) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)outSteps * cols) return;
  const float m = margin[g];
  const size_t stride = (size_t)outSteps * cols;
  long long n = 0, covered = 0;
  for (int r = 0; r < rows; ++r) {
    const float v = scores[(size_t)r * stride + g];
    n += v == v;
    covered += v <= m;                                               // false for a NaN on either side
  }
  counts[2 * g] = (accumulate ? counts[2 * g] : 0) + n;
  counts[2 * g + 1] = (accumulate ? counts[2 * g + 1] : 0) + covered;
}

// per horizon: one workgroup per horizon, integer partial counts added through LDS
__global__ __launch_bounds__(256) void k_conformal_coverage_rows(const float* __restrict__ scores, int rows, int outSteps,
                                                                 int cols, const float* __restrict__ margin, int accumulate,
                                                                 long long* __restrict__ counts) {
  __shared__ long long red[2 * 256];
  const int tid = threadIdx.x, o = blockIdx.x;
  const float m = margin[o];
  const int elems = rows * cols;                                      // < 2^31 (checked on the host)
  const float* src = scores + (size_t)o * cols;
  const size_t stride = (size_t)outSteps * cols;
  long long n = 0, covered = 0;
  for (int i = tid; i < elems; i += 256) {
    const int r = i / cols;
    const float v = src[(size_t)r * stride + (i - r * cols)];
    n += v == v;
    covered += v <= m;
  }
  red[2 * tid] = n; red[2 * tid + 1] = covered;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (tid < half) { red[2 * tid] += red[2 * (tid + half)]; red[2 * tid + 1] += red[2 * (tid + half) + 1]; }
    __syncthreads();
  }
  if (tid == 0) {
    counts[2 * o] = (accumulate ? counts[2 * o] : 0) + red[0];
    counts[2 * o + 1] = (accumulate ? counts[2 * o + 1] : 0) + red[1];
  }
}

// matgcn_region_loss.hip - the gradient of a training objective taken on region totals, handed back to the member nodes
// (matgcn_region_loss_grad, include/matgcn.h): the transpose of matgcn_group_sums.  Included by matgcn_capi.hip after
// matgcn_regions.hip and matgcn_loss.hip, whose loss_element / loss_slope / loss_term / LossArgs it uses unchanged.
//
// The value (matgcn_region_loss) has no kernel of its own beyond k_region_affine: it launches the total kernels of
// matgcn_regions.hip into the scratch and k_loss_partial / k_loss_final on the two total tensors with an identity affine.
//
// Coefficient of a region element (r, g, c), from the totals P, L in scratch: q = fp32(slope * keep), k_loss_grad's g before
// its final scaling (0 where the forward replaced a NaN term by 0; RMSE: divided by 2 rmse, all 0 when rmse == 0), rounded
// to fp32 ONCE.  The rounding is deliberate: (double)w * (double)q is then exact in fp64, so a contracted fma gives the bits
// of multiply then add - the idiom of matgcn_group_sums - and no compiler flag decides the result.
// Gradient of an element (r, n, c): one thread owns the chain from end to end.  It starts from 0.0 in fp64 and adds
// (double)weight[e] * (double)q[r, group[e], c] over the memberships e = ptr[n] .. ptr[n + 1] - 1 of the by-node map, which
// lists them in ascending member position of the by-group map; then part = ((double)upstream * (double)std) * acc / cnt
// (cnt == 0: part = 0) and d_pred = fp32(part), or fp32((double)base + part).  A node in no region gets base's bits, or +0.0.
// No atomics, no scratch written, nothing depends on the order workgroups run in.
//   - k_region_grad_tile: a workgroup of 256 threads takes R consecutive rows.  It computes the rows' G * od coefficients
//     once (a contiguous, coalesced read of the totals) into LDS, at most REGION_Q_FLOATS of them (32 KB); then thread t
//     takes the elements t, t + 256, .. of the tile's contiguous run of d_pred, so the store (and the read of base) is
//     coalesced along (n, c) and a chain reads LDS only.  The by-node map - group indices as element offsets, weights - is
//     staged behind the coefficients when it is at most 16 KB (REGION_MAP_FLOATS, the forward's budget: 48 KB in all, no
//     opt-in); a larger one is read from global memory through the caches: same chain, same bits.  A chain fetches its
//     memberships REGION_AHEAD at a time before it adds them, still one at a time and in listed order.
//   - k_region_grad_walk: G * od above REGION_Q_FLOATS - no tile holds one row's coefficients.  One thread per element;
//     the coefficient of each membership is recomputed from the totals in global memory.  The same chain.
// A group index outside 0 .. G-1 is clamped, as the forward clamps node indices: no map makes a kernel read outside the
// totals.

constexpr int REGION_Q_FLOATS = 8192;                  // 32 KB of LDS: the coefficients of a tile; a longer row is walked
constexpr int REGION_MAP_FLOATS = GROUP_MAP_FLOATS;    // a by-node map of up to 16 KB (offsets, weights) is staged beside them
constexpr int REGION_TILE_ELEMS = 4096;                // elements of d_pred in a tile of several rows: 16 per thread
constexpr int REGION_MAX_ROWS = 64;                    // rows of a tile
constexpr int REGION_MIN_TILES = 512;                  // rows per tile are halved while fewer tiles than this would run
constexpr int REGION_AHEAD = GROUP_AHEAD;              // memberships of a chain fetched before they are added
constexpr int REGION_THREADS = 256;

// the descriptor's scalar affine where the total kernels read it: two floats of the scratch
__global__ void k_region_affine(float* __restrict__ dst, float mean, float std) {
  if (threadIdx.x == 0) { dst[0] = mean; dst[1] = std; }
}

struct RegionGradArgs {
  LossArgs id;             // pred = P, lab.y = L: the totals (rows, G, od); mean 0, std 1; the descriptor's nullVal, minS, delta
  const double* kept;      // what k_loss_final left: the kept count, the fp64 mse
  const float* upstream;
  const float* base;       // (rows, N, od) or null; may be dpred
  float* dpred;            // (rows, N, od)
  long long rows;
  int N, od, rowLen;       // rowLen = N * od
  int G, GC;               // GC = G * od
  int R;                   // rows per tile
  int staged;              // the by-node map is copied into LDS behind the coefficients
  int members;
  float std;
  const int* nptr;         // device, N + 1
  const int* ngroup;       // device, members: group indices
  const float* nweight;    // device, members, or null = 1
};

template <int KIND, int MASKED>
__device__ __forceinline__ float region_coeff(const LossArgs& id, float P, float L, double cnt, double rmse) {
  float p, l, d;
  const bool keep = loss_element<MASKED>(id, L, P, p, l, d);
  const double delta = (double)id.delta;
  double g = 0.0;
  if (keep && cnt > 0.0) {
    g = loss_slope<KIND>(p, l, d, delta);
    if (MASKED) {
      const double t = loss_term<KIND>(p, l, d, delta);
      if (t != t) g = 0.0;                                // the forward replaced this term by 0
    }
    if (KIND == MATGCN_LOSS_RMSE) g = rmse > 0.0 ? g / (2.0 * rmse) : 0.0;
  }
  return (float)g;
}

// One chain: memberships k0 .. k1-1 in ascending k.  STAGED: `grp` holds element offsets (clamped group index times channel
// count, in LDS); otherwise the map's raw group indices.  TILE: q points at the coefficients (row, channel) of the tile in
// LDS; otherwise the coefficient at offset o is recomputed from the totals at rowAt + o.  The fetches of REGION_AHEAD
// memberships are independent of each other and of the sum; the adds are not reordered.  A slot behind the end re-reads
// membership k1 - 1 and is not added.
template <int KIND, int MASKED, bool TILE, bool STAGED>
__device__ __forceinline__ double region_chain(const RegionGradArgs& a, const int* grp, const float* wgt, int k0, int k1,
                                               const float* q, size_t rowAt, double cnt, double rmse) {
  double acc = 0.0;
  for (int k = k0; k < k1; k += REGION_AHEAD) {
    int o[REGION_AHEAD];
    float w[REGION_AHEAD], v[REGION_AHEAD];
#pragma unroll
    for (int u = 0; u < REGION_AHEAD; ++u) {
      const int kk = k + u < k1 ? k + u : k1 - 1;
      o[u] = grp[kk];
      if (!STAGED) o[u] = (o[u] < 0 ? 0 : (o[u] >= a.G ? a.G - 1 : o[u])) * a.od;
      w[u] = wgt ? wgt[kk] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < REGION_AHEAD; ++u) {
      if (TILE) {
        v[u] = q[o[u]];
      } else {
        v[u] = k + u < k1 ? region_coeff<KIND, MASKED>(a.id, a.id.pred[rowAt + o[u]], a.id.lab.y[rowAt + o[u]], cnt, rmse) : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < REGION_AHEAD; ++u)
      if (k + u < k1) acc += (double)w[u] * (double)v[u];
  }
  return acc;
}

// the element from its chain: fp32(part), or fp32(base + part)
__device__ __forceinline__ float region_store(double acc, double scale, double cnt, const float* base, size_t idx) {
  const double part = cnt > 0.0 ? scale * acc / cnt : 0.0;
  return base ? (float)((double)base[idx] + part) : (float)part;
}

template <int KIND, int MASKED>
__global__ __launch_bounds__(REGION_THREADS) void k_region_grad_tile(RegionGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float regionTile[];
  const int tid = threadIdx.x, rowLen = a.rowLen, od = a.od, GC = a.GC;
  const long long row0 = (long long)blockIdx.x * a.R;
  const long long left = a.rows - row0;
  const int nRows = left < a.R ? (int)left : a.R;
  const double cnt = MASKED ? a.kept[0] : (double)a.rows * (double)GC;
  const double rmse = KIND == MATGCN_LOSS_RMSE ? sqrt(a.kept[1]) : 0.0;
  // ---- the coefficients of the tile's rows, once --------------------------------------------------------------------------
  {
    const size_t at = (size_t)row0 * GC;
    const int nq = nRows * GC;                                       // <= REGION_Q_FLOATS
    for (int i = tid; i < nq; i += REGION_THREADS)
      regionTile[i] = region_coeff<KIND, MASKED>(a.id, a.id.pred[at + i], a.id.lab.y[at + i], cnt, rmse);
  }
  // ---- the by-node map, where it fits behind them ---------------------------------------------------------------------------
  int* mapGroup = reinterpret_cast<int*>(regionTile + a.R * GC);
  float* mapWeight = a.nweight ? regionTile + a.R * GC + a.members : nullptr;
  if (a.staged) {
    for (int k = tid; k < a.members; k += REGION_THREADS) {
      const int g = a.ngroup[k];
      mapGroup[k] = (g < 0 ? 0 : (g >= a.G ? a.G - 1 : g)) * od;
      if (a.nweight) mapWeight[k] = a.nweight[k];
    }
  }
  __syncthreads();
  // ---- the chains: thread t owns the elements t, t + 256, .. of the tile's contiguous run ------------------------------------
  const double scale = (double)a.upstream[0] * (double)a.std;
  const int count = nRows * rowLen;                                  // <= REGION_TILE_ELEMS, or one row: < 2^31 (host check)
  for (int e = tid; e < count; e += REGION_THREADS) {
    const int r = e / rowLen, j = e - r * rowLen;
    const int n = od == 1 ? j : j / od, c = j - n * od;
    const int k0 = a.nptr[n], k1 = a.nptr[n + 1];
    const size_t idx = (size_t)(row0 + r) * rowLen + j;
    float out;
    if (k1 <= k0) {                                                  // a node in no region: base's bits, or +0.0
      out = a.base ? a.base[idx] : 0.f;
    } else {
      const float* q = regionTile + r * GC + c;
      const double acc = a.staged
          ? region_chain<KIND, MASKED, true, true>(a, mapGroup, mapWeight, k0, k1, q, 0, cnt, rmse)
          : region_chain<KIND, MASKED, true, false>(a, a.ngroup, a.nweight, k0, k1, q, 0, cnt, rmse);
      out = region_store(acc, scale, cnt, a.base, idx);
    }
    a.dpred[idx] = out;
  }
}

template <int KIND, int MASKED>
__global__ __launch_bounds__(REGION_THREADS) void k_region_grad_walk(RegionGradArgs a, long long total) {
  const long long idx = (long long)blockIdx.x * REGION_THREADS + threadIdx.x;
  if (idx >= total) return;
  const long long row = idx / a.rowLen;
  const int j = (int)(idx - row * a.rowLen);
  const int n = j / a.od, c = j - n * a.od;
  const double cnt = MASKED ? a.kept[0] : (double)a.rows * (double)a.GC;
  const double rmse = KIND == MATGCN_LOSS_RMSE ? sqrt(a.kept[1]) : 0.0;
  const int k0 = a.nptr[n], k1 = a.nptr[n + 1];
  float out;
  if (k1 <= k0) {
    out = a.base ? a.base[idx] : 0.f;
  } else {
    const double acc = region_chain<KIND, MASKED, false, false>(a, a.ngroup, a.nweight, k0, k1, nullptr,
                                                                (size_t)row * a.GC + c, cnt, rmse);
    out = region_store(acc, (double)a.upstream[0] * (double)a.std, cnt, a.base, (size_t)idx);
  }
  a.dpred[idx] = out;
}

// matgcn_regions.hip - totals over groups of nodes ("regions": counties, districts, corridors) of a (rows, N, od) tensor on
// the re-transformed scale (matgcn_group_sums) and of the labels of a batch (matgcn_group_label_sums; include/matgcn.h).
// Included by matgcn_capi.hip after matgcn_kernels.hip, whose descriptor (NodeScale, descale_node) it uses unchanged.
//
// A region map is a CSR list over groups.  One thread owns one (row, group, channel) chain from its first member to its
// last: it starts from 0.0 in fp64, adds (double)weight[k] * (double)v(node[k]) for k = ptr[g] .. ptr[g + 1] - 1 in
// ascending k, one member at a time, and rounds to fp32 once.  The product of two fp32 values is exact in fp64, so the
// bits do not depend on whether the compiler contracts the multiply and the add.  No chain is ever split: no atomics, no
// scratch, and nothing depends on the order workgroups run in.
//   - k_group_sums_tile: a workgroup of 256 threads takes R consecutive rows, reads them from HBM once as one contiguous
//     run (16-byte loads where the run is aligned), de-scales and clamps on load and keeps them in LDS; the chains then walk
//     LDS.  Adjacent lanes hold adjacent rows of one (group, channel): their chains have the same length, their node and
//     weight loads are wave-uniform, and the odd row stride in LDS puts them on different banks.  A tile of several rows
//     is at most 8 192 floats (32 KB: five workgroups share a CU and hide each other's load latency; R = 20 at N = 403,
//     od = 1), a single row up to 16 384 (64 KB, no opt-in: R = 1 at N = 4096, od = 2).
//   - Both phases are latency-bound when written naively - a chain is a dependent walk of index load, value read and add.
//     So the row loads are issued four 16-byte loads ahead, and a chain fetches its members GROUP_AHEAD at a time
//     (indices, then weights and values) before it adds them, still one at a time and in listed order; and a map of up to
//     16 KB is copied into LDS behind the rows once per workgroup, as element offsets, so a chain never waits for global
//     memory (a larger map is read from global memory through the caches: same chain, same bits).
//   - k_group_walk: a row of more than 16 384 floats, and the labels of a batch (strided, gathered rows; a small tensor):
//     the same chain with its members read from global memory and de-scaled as they are met.
// A node index outside 0 .. N-1 is clamped into the row: a map is validated where it is built, but no index may make a
// kernel read outside the tensor.

constexpr int GROUP_TILE_FLOATS = 16384;     // 64 KB of LDS: the longest row a tile holds
constexpr int GROUP_ROWS_FLOATS = 8192;      // a tile of several rows
constexpr int GROUP_MAP_FLOATS = 4096;       // a map of up to 16 KB (offsets, weights) is staged beside the rows
constexpr int GROUP_AHEAD = 8;               // members of a chain fetched before they are added
constexpr int GROUP_MAX_ROWS = 256;          // rows of a tile
constexpr int GROUP_THREADS = 256;

struct GroupMap {
  const int* ptr;        // device, G + 1
  const int* node;       // device, members
  const float* weight;   // device, members, or null = 1
  int G;
};

// the member arithmetic: both affines, then the clamp from below (NaN: off; a NaN value stays NaN)
__device__ __forceinline__ float group_member(const NodeScale& sc, int n, float v) {
  v = descale_node(sc, n, v);
  if (sc.clampMin == sc.clampMin && v < sc.clampMin) v = sc.clampMin;
  return v;
}
__device__ __forceinline__ int group_node(const GroupMap& m, int k, int N) {
  const int n = m.node[k];
  return n < 0 ? 0 : (n >= N ? N - 1 : n);
}

// One chain: members k0 .. k1-1 of the map in ascending k.  STAGED: `node` holds element offsets (clamped index times
// channel count, written by the workgroup into LDS) and x the tile's member values; otherwise `node` holds the map's raw
// indices, the value of node n is x[n * nodeStride] and is de-scaled on the way.  The fetches of GROUP_AHEAD members are
// independent of each other and of the sum; the adds are not reordered.  A slot behind the end re-reads member k1 - 1 and
// is not added.
template <bool STAGED>
__device__ __forceinline__ float group_chain(const int* node, const float* weight, const NodeScale& sc, int N, int k0, int k1,
                                             const float* x, size_t nodeStride) {
  double acc = 0.0;
  for (int k = k0; k < k1; k += GROUP_AHEAD) {
    int n[GROUP_AHEAD];
    float w[GROUP_AHEAD], v[GROUP_AHEAD];
#pragma unroll
    for (int u = 0; u < GROUP_AHEAD; ++u) {
      const int kk = k + u < k1 ? k + u : k1 - 1;
      n[u] = node[kk];
      if (!STAGED) n[u] = n[u] < 0 ? 0 : (n[u] >= N ? N - 1 : n[u]);
      w[u] = weight ? weight[kk] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < GROUP_AHEAD; ++u) {
      if (STAGED) {
        v[u] = x[n[u]];
      } else {
        v[u] = group_member(sc, n[u], x[(size_t)n[u] * nodeStride]);
      }
    }
#pragma unroll
    for (int u = 0; u < GROUP_AHEAD; ++u)
      if (k + u < k1) acc += (double)w[u] * (double)v[u];
  }
  return (float)acc;
}

struct GroupTileArgs {
  const float* values;   // (rows, N, od)
  long long rows;
  int N, od, rowLen;     // rowLen = N * od
  int stride;            // rowLen | 1: the row stride of the tile in LDS
  int R;                 // rows per tile
  int mapAt;             // >= 0: the map's element offsets (and weights) are staged in LDS from this float of the tile on
  int members;
  int stepQuot, stepRem; // 4 * GROUP_THREADS = stepQuot * rowLen + stepRem
  NodeScale sc;
  GroupMap map;
  float* out;            // (rows, G, od)
};

__global__ __launch_bounds__(GROUP_THREADS) void k_group_sums_tile(GroupTileArgs a) {
  extern __shared__ __attribute__((aligned(16))) float groupTile[];
  const int tid = threadIdx.x, rowLen = a.rowLen, od = a.od;
  const long long row0 = (long long)blockIdx.x * a.R;
  const long long left = a.rows - row0;
  const int nRows = left < a.R ? (int)left : a.R;
  const float* src = a.values + (size_t)row0 * rowLen;
  const int count = nRows * rowLen;                                  // <= GROUP_TILE_FLOATS
  // ---- the rows, once: element idx of the run is row idx / rowLen, position idx % rowLen -------------------------------
  const int nVec = (reinterpret_cast<size_t>(src) & 15) == 0 ? count >> 2 : 0;
  {
    int idx = 4 * tid;
    int r = idx / rowLen, j = idx - r * rowLen;
    for (; idx < 4 * nVec; idx += 16 * GROUP_THREADS) {
      float4 q[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {                                  // four loads in flight; behind the end: the first again
        const int at = idx + p * 4 * GROUP_THREADS;
        q[p] = *reinterpret_cast<const float4*>(src + (at < 4 * nVec ? at : idx));
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (idx + p * 4 * GROUP_THREADS < 4 * nVec) {
          const float v[4] = {q[p].x, q[p].y, q[p].z, q[p].w};
          int rr = r, jj = j;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            while (jj >= rowLen) { jj -= rowLen; ++rr; }             // at most 3 turns in all (idx + u < count)
            const int n = od == 1 ? jj : jj / od;
            groupTile[rr * a.stride + jj] = group_member(a.sc, n, v[u]);
            ++jj;
          }
        }
        j += a.stepRem; r += a.stepQuot;
        if (j >= rowLen) { j -= rowLen; ++r; }
      }
    }
  }
  for (int idx = 4 * nVec + tid; idx < count; idx += GROUP_THREADS) {
    const int r = idx / rowLen, j = idx - r * rowLen;
    const int n = od == 1 ? j : j / od;
    groupTile[r * a.stride + j] = group_member(a.sc, n, src[idx]);
  }
  // ---- the map, where it fits beside the rows: every chain of the workgroup walks it ------------------------------------
  int* mapNode = reinterpret_cast<int*>(groupTile + (a.mapAt >= 0 ? a.mapAt : 0));
  float* mapWeight = a.map.weight ? groupTile + a.mapAt + a.members : nullptr;
  if (a.mapAt >= 0) {
    for (int k = tid; k < a.members; k += GROUP_THREADS) {
      mapNode[k] = group_node(a.map, k, a.N) * od;
      if (a.map.weight) mapWeight[k] = a.map.weight[k];
    }
  }
  __syncthreads();
  // ---- the chains: row fastest, so a wave walks one member list -----------------------------------------------------------
  const int chains = a.map.G * od * nRows;                           // < 2^31 (host check)
  for (int ch = tid; ch < chains; ch += GROUP_THREADS) {
    const int gc = ch / nRows, r = ch - gc * nRows;
    const int g = gc / od, c = gc - g * od;
    const int k0 = a.map.ptr[g], k1 = a.map.ptr[g + 1];
    const float* x = groupTile + r * a.stride + c;
    float total;
    if (a.mapAt >= 0) {
      total = group_chain<true>(mapNode, mapWeight, a.sc, a.N, k0, k1, x, 0);
    } else {                                                         // the tile holds member values: nothing left to de-scale
      NodeScale none;
      none.mean = none.std = none.mean2 = none.std2 = nullptr; none.perNode = 0; none.clampMin = __builtin_nanf("");
      total = group_chain<false>(a.map.node, a.map.weight, none, a.N, k0, k1, x, (size_t)od);
    }
    a.out[((size_t)(row0 + r) * a.map.G + g) * od + c] = total;
  }
}

struct GroupWalkArgs {
  // the argument order from before LabelView (k_group_walk measured slower with the view embedded: DESIGN.md 5f)
  const float* src;        // values (rows, N, od), or labels: windows (B, ySteps, N, yFeat) / the raw series (ySteps, N, yFeat)
  const int* labelStart;   // labels over the series, else null
  int labels;              // 1: src holds labels, row = b * outSteps + o
  int outSteps, ySteps, yFeat, yStart;
  int N, od;
  long long total;         // rows * G * od chains
  NodeScale sc;
  GroupMap map;
  float* out;              // (rows, G, od)
};

__global__ __launch_bounds__(GROUP_THREADS) void k_group_walk(GroupWalkArgs a) {
  const long long ch = (long long)blockIdx.x * GROUP_THREADS + threadIdx.x;
  if (ch >= a.total) return;
  const long long gc = ch / a.od;
  const int c = (int)(ch - gc * a.od);
  const long long row = gc / a.map.G;
  const int g = (int)(gc - row * a.map.G);
  const float* x;
  int nodeStride;
  if (a.labels) {
    const LabelView v = {a.src, a.labelStart, a.outSteps, a.N, a.od, a.ySteps, a.yFeat, a.yStart};
    const long long b = row / a.outSteps;
    x = label_ptr(v, label_row(v, b, (int)(row - b * a.outSteps)), 0) + c;
    nodeStride = a.yFeat;
  } else {
    x = a.src + (size_t)row * a.N * a.od + c;
    nodeStride = a.od;
  }
  a.out[ch] = group_chain<false>(a.map.node, a.map.weight, a.sc, a.N, a.map.ptr[g], a.map.ptr[g + 1], x, (size_t)nodeStride);
}

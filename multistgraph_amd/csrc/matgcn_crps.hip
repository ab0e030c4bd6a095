// matgcn_crps.hip - the CRPS of a Monte-Carlo-dropout ensemble as a training objective, value and gradient
// (matgcn_crps_loss / matgcn_crps_loss_grad, include/matgcn.h).  Included by matgcn_capi.hip behind matgcn_mc_scores.hip
// and matgcn_loss.hip, whose pieces it is made of:
//   - samples (S, B, out, N, od), labels, mask and de-scaling are those of k_mc_scores; the sort is its LDS bitonic network
//     with its tile rule (mc_tile: 64 / 32 / 16 elements by S), the value of an element its expression
//     c = A / S - W / S^2 with A = sum_s |p_s - l| and W = sum_i (2i - S + 1) p_(i), fp64 from the fp32 values;
//   - the two stages, the scratch (2*B*out + 2 doubles) and the rule for a group that keeps nothing are those of
//     matgcn_loss: stage 2 IS k_loss_final<MATGCN_LOSS_MAE>, which also leaves the count M for the gradient.
// Value: one workgroup per (b, horizon) row; it walks the row's tiles in ascending order, wave 0 owns one element per lane
// and adds its terms tile after tile, then folds its lanes by halves.  Gradient: one workgroup per tile; (value, sample)
// pairs are sorted - ties by sample index, so the rank r_s of every sample is a definite number - and position i of the
// sorted column writes d_samples[s_(i)] = upstream * (std / M) * (sgn(p - l) / S - (2i - S + 1) / S^2), rounded once.
// A tile is read completely (into LDS) before anything of it is written, and no other workgroup touches its elements:
// d_samples may be the samples.  The rows S .. P-1 of the padding carry the indices S .. P-1: they sort behind equal
// values and are never written.  No atomics, nothing allocated, no result depends on the order the workgroups run in.

struct CrpsArgs {
  const float* samples;   // (S, B, out, N, od)
  LabelView lab;
  int S, P, logTE, tilesPerRow;
  long long E;
  float mean, std, nullVal, minS;
};

// the label of element (n, c) of row (b, o), de-scaled and filtered as in k_mc_scores; false where the mask drops it
__device__ __forceinline__ bool crps_label(const CrpsArgs& a, size_t yrow, int r, float& l) {
  const int n = r / a.lab.od, c = r - n * a.lab.od;
  l = scale_affine(label_at(a.lab, yrow, n, c), a.std, a.mean);
  if (fabsf(l) < a.minS) l = 0.f;
  return a.nullVal != a.nullVal ? l == l : l != a.nullVal;
}

// stage 1: scratch[2 * row] = sum of the kept elements' CRPS of row (b, o), scratch[2 * row + 1] = the kept elements
__global__ __launch_bounds__(256) void k_crps_partial(CrpsArgs a, double* __restrict__ scratch) {
  extern __shared__ __attribute__((aligned(16))) float mcTile[];
  const int logTE = a.logTE, TE = 1 << logTE, tid = threadIdx.x, S = a.S;
  const int rowLen = a.lab.N * a.lab.od;
  const int row = blockIdx.x, b = row / a.lab.outSteps, o = row - b * a.lab.outSteps;
  const int e = tid & (TE - 1), slot = tid >> logTE, slots = 256 >> logTE;
  const size_t yrow = label_row(a.lab, (size_t)b, o);
  const double Sd = (double)S;
  double sTerm = 0.0, sCnt = 0.0;                         // threads tid < TE: the elements e, e + TE, .. of the row
  for (int t = 0; t < a.tilesPerRow; ++t) {
    const int r0 = t << logTE;
    const int nValid = min(TE, rowLen - r0);
    mc_sort_tile(mcTile, a.samples, S, a.P, logTE, (size_t)a.E, (size_t)row * rowLen + r0, nValid, a.mean, a.std);
    float l = 0.f;
    const bool keep = e < nValid && crps_label(a, yrow, r0 + e, l);
    const double ld = (double)l;
    double sAbs = 0.0, sWgt = 0.0;
    for (int i = slot; i < S; i += slots) {
      const double xi = (double)mcTile[(mc_row(i) << logTE) + e];
      sAbs += fabs(xi - ld);
      sWgt += mc_mul((double)(2 * i - S + 1), xi);        // exact: an integer below 2^11 times an fp32 value
    }
    __syncthreads();                                      // the sorted tile has been read: its floats become the scratch
    double* red = reinterpret_cast<double*>(mcTile);
    red[2 * tid] = sAbs; red[2 * tid + 1] = sWgt;
    __syncthreads();
    if (tid < TE && keep) {
      double A = 0.0, W = 0.0;
      for (int s = 0; s < slots; ++s) { A += red[2 * ((s << logTE) + e)]; W += red[2 * ((s << logTE) + e) + 1]; }
      sCnt += 1.0;
      sTerm += A / Sd - W / (Sd * Sd);
    }
    __syncthreads();                                      // ... and are free for the next tile
  }
  if (tid >= 64) return;                                  // wave 0 holds every element (TE <= 64)
  for (int sh = 32; sh > 0; sh >>= 1) { sTerm += __shfl_down(sTerm, sh, 64); sCnt += __shfl_down(sCnt, sh, 64); }
  if (tid == 0) { scratch[2 * (size_t)row] = sTerm; scratch[2 * (size_t)row + 1] = sCnt; }
}

// the network of mc_sort_network over (value, sample index) pairs: ascending by value, equal values by index
__device__ __forceinline__ void crps_sort_pairs(float* __restrict__ x, unsigned short* __restrict__ ix, int P, int logTE) {
  const int TE = 1 << logTE, tid = threadIdx.x;
  __syncthreads();
  const int pairs = (P >> 1) << logTE;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = tid; idx < pairs; idx += 256) {
        const int pr = idx >> logTE, e = idx & (TE - 1);
        const int i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), l = i | j;   // i < l < P
        const int pa = (mc_row(i) << logTE) + e, pb = (mc_row(l) << logTE) + e;
        const float va = x[pa], vb = x[pb];
        const unsigned short ia = ix[pa], ib = ix[pb];
        const bool above = va > vb || (va == vb && ia > ib);
        if (above == ((i & k) == 0)) { x[pa] = vb; x[pb] = va; ix[pa] = ib; ix[pb] = ia; }
      }
      __syncthreads();
    }
  }
}

// d result[0] / d samples; kept[0] = the count M that k_loss_final left behind the slabs of the value call
__global__ __launch_bounds__(256) void k_crps_grad(CrpsArgs a, const double* __restrict__ kept, float upstream,
                                                   float* __restrict__ dSamples) {
  extern __shared__ __attribute__((aligned(16))) float mcTile[];
  const int logTE = a.logTE, TE = 1 << logTE, tid = threadIdx.x, S = a.S, P = a.P;
  unsigned short* ix = reinterpret_cast<unsigned short*>(mcTile + ((size_t)P << logTE));
  const int rowLen = a.lab.N * a.lab.od;
  const int row = blockIdx.x / a.tilesPerRow, t = blockIdx.x - row * a.tilesPerRow;
  const int b = row / a.lab.outSteps, o = row - b * a.lab.outSteps;
  const int r0 = t << logTE;
  const int nValid = min(TE, rowLen - r0);
  const size_t E = (size_t)a.E, e0 = (size_t)row * rowLen + r0;
  const int e = tid & (TE - 1);                           // 256 is a multiple of TE: a thread owns one column
  const bool inRow = e < nValid;
  for (int s = tid >> logTE; s < P; s += 256 >> logTE) {
    float v = __builtin_inff();
    if (!inRow) v = 0.f;
    else if (s < S) v = scale_affine(a.samples[(size_t)s * E + e0 + e], a.std, a.mean);
    const int at = (mc_row(s) << logTE) + e;
    mcTile[at] = v; ix[at] = (unsigned short)s;
  }
  crps_sort_pairs(mcTile, ix, P, logTE);
  if (!inRow) return;
  float l = 0.f;
  const bool keep = crps_label(a, label_row(a.lab, (size_t)b, o), r0 + e, l);
  const double M = kept[0], Sd = (double)S, ld = (double)l;
  const bool live = keep && M > 0.0;
  const double w = live ? (double)upstream * (double)a.std / M : 0.0;
  for (int i = tid >> logTE; i < P; i += 256 >> logTE) {
    const int at = (mc_row(i) << logTE) + e;
    const int s = ix[at];
    if (s >= S) continue;                                 // padding
    double g = 0.0;
    if (live) g = w * (loss_sign((double)mcTile[at] - ld) / Sd - (double)(2 * i - S + 1) / (Sd * Sd));
    dSamples[(size_t)s * E + e0 + e] = (float)g;
  }
}

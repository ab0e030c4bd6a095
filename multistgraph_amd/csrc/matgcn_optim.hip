// matgcn_optim.hip - the tail of a training step on the device: global gradient norm, clip and Adam over a table of
// tensors (matgcn_grad_norm / matgcn_adam_step, include/matgcn.h).  Included by matgcn_capi.hip.
//
// Index space: every tensor is cut into chunks of OPT_CHUNK = 4096 elements, the last one short; a chunk never straddles
// two tensors.  One workgroup of 256 threads takes one chunk; thread t owns the elements 4 t .. 4 t + 3 of each of the
// four 1024-element slabs of the chunk (a float4 per slab where the pointers allow it, four scalar accesses otherwise -
// the same elements either way, so no result depends on the alignment of a view).
// The table of a launch - at most OPT_MAX_TENSORS tensors, their four pointers, sizes and chunk prefix sums - travels by
// value in the kernel arguments (2.8 KB of the 4 KB a launch carries): no device copy of it exists, so there is nothing to
// upload per step and nothing to keep alive.  A workgroup finds its tensor by a binary search over the prefix sums; the
// index is uniform, so the search and the table reads are scalar loads from the kernarg segment.  More tensors are more
// launches of the same kernels.
// Nothing is allocated, no atomics, nothing depends on the order the workgroups run in.  No index depends on data: a
// non-finite gradient reaches the elements it belongs to and nothing else.
//
// Arithmetic whose order the header promises is written one rounding per statement with contraction switched off, as in
// matgcn_mc_scores.hip; `/` and sqrtf are the correctly rounded ones (hipcc's default, no fast-math in the build flags).
// The table is 2.8 KB of the kernel arguments, the scalars another 48 bytes.

constexpr int OPT_CHUNK = 4096;
constexpr int OPT_MAX_TENSORS = 64;
constexpr int OPT_THREADS = 256;
constexpr int OPT_SUM_TILE = 2048;                      // k_opt_norm_finish: partials staged in LDS per round

struct OptTable {
  float* param[OPT_MAX_TENSORS];
  const float* grad[OPT_MAX_TENSORS];
  float* expAvg[OPT_MAX_TENSORS];
  float* expAvgSq[OPT_MAX_TENSORS];
  long long numel[OPT_MAX_TENSORS];
  int chunkEnd[OPT_MAX_TENSORS];                        // chunks of the tensors 0 .. i of this launch (ascending; empty tensors repeat)
  int n;                                                // tensors in this launch (1 .. OPT_MAX_TENSORS)
};

struct OptScalars {
  double w1, w2;         // 1 - beta1, 1 - beta2
  double beta2;
  double weightDecay;
  float stepSize;        // (float)(lr / (1 - beta1^step))
  float bc2Sqrt;         // (float)sqrt(1 - beta2^step)
  float eps;
  float maxNorm;         // > 0: clip
};

// the tensor of chunk `c`: the first i with c < chunkEnd[i] (c < chunkEnd[n - 1] by the size of the grid)
__device__ __forceinline__ int opt_find(const OptTable& T, int c) {
  int lo = 0, hi = T.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c < T.chunkEnd[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ bool opt_aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// launch 1: partials[chunkBase + block] = sum of g^2 over the chunk, in fp64.  Order: thread t adds its 16 elements in
// ascending index; the 64 lanes of a wave fold by halves (lane l += lane l + 32, 16, .. 1); thread 0 adds the four waves
// in ascending order.
__global__ __launch_bounds__(OPT_THREADS) void k_opt_sumsq(OptTable T, int chunkBase, double* __restrict__ partials) {
  __shared__ double waveSum[OPT_THREADS / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int t = opt_find(T, c);
  const long long first = (long long)(c - (t ? T.chunkEnd[t - 1] : 0)) * OPT_CHUNK;
  const long long left = T.numel[t] - first;            // >= 1
  const int len = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  const float* __restrict__ g = T.grad[t] + first;
  const bool vec = opt_aligned16(T.grad[t]);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < OPT_CHUNK / (4 * OPT_THREADS); ++k) {
    const int i = k * 4 * OPT_THREADS + 4 * tid;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec && i + 4 <= len) {
      const float4 q = *reinterpret_cast<const float4*>(g + i);
      x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (i + j < len) x[j] = g[i + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
      const double d = (double)x[j];
      const double sq = d * d;                           // exact: 48 bits of product
      s = s + sq;
    }
  }
  for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_down(s, sh, 64);
  if ((tid & 63) == 0) waveSum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partials[(size_t)chunkBase + c] = ((waveSum[0] + waveSum[1]) + waveSum[2]) + waveSum[3];
}

// launch 2: one workgroup; total_norm = (float)sqrt(partials[0] + partials[1] + ..), added in ascending index by one
// thread.  The other threads only stage the partials in LDS, OPT_SUM_TILE at a time, so that the chain of dependent
// additions waits for LDS and not for HBM.
__global__ __launch_bounds__(OPT_THREADS) void k_opt_norm_finish(const double* __restrict__ partials, int chunks,
                                                                 float* __restrict__ totalNorm) {
  __shared__ double tile[OPT_SUM_TILE];
  double sum = 0.0;
  for (int base = 0; base < chunks; base += OPT_SUM_TILE) {
    const int m = min(OPT_SUM_TILE, chunks - base);
    for (int i = threadIdx.x; i < m; i += OPT_THREADS) tile[i] = partials[(size_t)base + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) sum += tile[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) *totalNorm = (float)sqrt(sum);
}

// One element of the update.  The two moments are formed in fp64 from the fp32 values and rounded once each - the clip
// coefficient is common to every element and g enters exp_avg_sq squared, so in fp32 its one rounding would come back
// doubled in all of them at once; the additions and products below are exact or nearly so in fp64 and cost nothing next
// to the seven memory accesses.  The parameter then moves as in torch's _single_tensor_adam, in fp32 from the rounded
// moments, one rounding per line.
__device__ __forceinline__ void opt_adam_element(float& p, float g, float& m, float& v, double coef, const OptScalars& h) {
#pragma clang fp contract(off)
  double gd = (double)g * coef;
  if (h.weightDecay != 0.0) {
    const double t = h.weightDecay * (double)p;
    gd = gd + t;
  }
  const double md = (double)m;                           // exp_avg.lerp_(g, 1 - beta1)
  const double d = gd - md;
  const double wd = h.w1 * d;
  m = (float)(md + wd);
  const double bv = h.beta2 * (double)v;                 // exp_avg_sq.mul_(beta2).addcmul_(g, g, value = 1 - beta2)
  const double wg = h.w2 * gd;
  const double wgg = wg * gd;
  v = (float)(bv + wgg);
  const float r = sqrtf(v);                              // denom = sqrt(v) / sqrt(bc2) + eps
  const float rs = r / h.bc2Sqrt;
  const float den = rs + h.eps;
  const float q = m / den;                               // param.addcdiv_(exp_avg, denom, value = -step_size)
  const float sq = h.stepSize * q;
  p = p - sq;
}

// launch 3: clip and Adam over the chunks of one table.  grad is read only.
__global__ __launch_bounds__(OPT_THREADS) void k_opt_adam(OptTable T, OptScalars h, const float* __restrict__ totalNorm) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const int t = opt_find(T, c);
  const long long first = (long long)(c - (t ? T.chunkEnd[t - 1] : 0)) * OPT_CHUNK;
  const long long left = T.numel[t] - first;
  const int len = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  float* __restrict__ p = T.param[t] + first;
  const float* __restrict__ g = T.grad[t] + first;
  float* __restrict__ m = T.expAvg[t] + first;
  float* __restrict__ v = T.expAvgSq[t] + first;
  const bool vec = opt_aligned16(T.param[t]) && opt_aligned16(T.grad[t]) && opt_aligned16(T.expAvg[t]) &&
                   opt_aligned16(T.expAvgSq[t]);
  double coef = 1.0;
  if (h.maxNorm > 0.f) {                                 // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1); NaN stays NaN
#pragma clang fp contract(off)
    const double nrm = (double)*totalNorm + 1e-6;
    coef = (double)h.maxNorm / nrm;
    coef = coef > 1.0 ? 1.0 : coef;
  }
#pragma unroll
  for (int k = 0; k < OPT_CHUNK / (4 * OPT_THREADS); ++k) {
    const int i = k * 4 * OPT_THREADS + 4 * tid;
    if (i >= len) break;
    if (vec && i + 4 <= len) {
      float4 P = *reinterpret_cast<const float4*>(p + i);
      const float4 G = *reinterpret_cast<const float4*>(g + i);
      float4 M = *reinterpret_cast<const float4*>(m + i);
      float4 V = *reinterpret_cast<const float4*>(v + i);
      opt_adam_element(P.x, G.x, M.x, V.x, coef, h);
      opt_adam_element(P.y, G.y, M.y, V.y, coef, h);
      opt_adam_element(P.z, G.z, M.z, V.z, coef, h);
      opt_adam_element(P.w, G.w, M.w, V.w, coef, h);
      *reinterpret_cast<float4*>(p + i) = P;
      *reinterpret_cast<float4*>(m + i) = M;
      *reinterpret_cast<float4*>(v + i) = V;
    } else {
      const int e = min(4, len - i);
      for (int j = 0; j < e; ++j) {
        float P = p[i + j], M = m[i + j], V = v[i + j];
        opt_adam_element(P, g[i + j], M, V, coef, h);
        p[i + j] = P; m[i + j] = M; v[i + j] = V;
      }
    }
  }
}

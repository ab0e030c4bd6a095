// matgcn_head_mc_bwd.hip - the transpose of k_head_mc: the output head's backward over S dropout samples
// (matgcn_backward_mc, include/matgcn.h).  Included by matgcn_capi.hip behind matgcn_kernels.hip.
//
// With d_s (B, CH, N) the gradient of sample s (channel ch = o*od + dd of the (S, B, out, N, od) tensor), W the plain
// end_conv weight (CH, hT, 64), seq the top layer's sequence and mask_s the multipliers of (seed, offset + s):
//   dSeq[b,t,n,h] = sum_s mask_s[b,t,n,h] * sum_c d_s[b,c,n] * W[c,t,h]                      (k_head_mc_dseq)
//   dW[c,t,h]     = sum_s sum_{b,n} d_s[b,c,n] * mask_s[b,t,n,h] * seq[b,t,n,h]              (k_head_mc_wgrad)
//   dBias[c]      = sum_s sum_{b,n} d_s[b,c,n]                                               (k_head_mc_dbias*)
// No mask and no per-sample tensor exists: a multiplier is drawn from matgcn_philox.h at the element's position in the
// logical (B, hT, N, 64) mask, the bit the forward drew there.  Both products run on the fp32 MFMA (32x32x2), fp32 in every
// training precision mode, as the head itself.
//
// k_head_mc_dseq: k_head_mc's shape - one workgroup of four waves per (b, 32-node tile), wave w owns the steps w, w + 4, ..
// (six at most: hT <= 24), its 6 x 64 x 32 outputs stay in 192 accumulator registers per lane over all samples and are
// stored once.  Per sample the workgroup stages the 32 x CH tile of d_s in LDS (double-buffered: one barrier per sample;
// the next sample's values are requested before the products of this one), a wave multiplies W_t^T (64 x CH, from L2) with
// it - rows = hidden channels, columns = nodes, so that a lane's four consecutive accumulator rows are one mask quad and
// one Philox call - and adds multiplier * product onto the accumulators.
//
// k_head_mc_wgrad: the reduction runs over (s, b, n).  A workgroup owns 32 channels (blockIdx.z) x 12 steps (blockIdx.y;
// three per wave: 96 accumulator registers) and walks its share of the (b, 32-node tile) items - blockIdx.x, .. + gridDim.x
// - and all samples of each with the accumulators in registers; the item's 3 x 32 x 64 slice of seq sits in 96 more
// registers over the samples.  Per sample: A = d_s^T (32 channels x 32 nodes, from the staged tile), B = mask_s * seq
// (32 nodes x 32 hidden channels per MFMA tile).  A lane of B holds ONE hidden channel of 16 nodes - one word of 16 mask
// quads - so the four lanes of an aligned quad share their calls: lane m draws the quads of the node pairs m, m + 4, m + 8,
// m + 12, packs the 4 x 4 keep bits, and the quad exchanges them (four shuffles per tile): 48 calls per lane and sample, as
// in the forward.  At the end every workgroup stores its tile of ONE partial slab [blockIdx.x][CH][hT][64] - no atomics -
// and k_ordered_reduce adds the slabs in ascending order: the weight gradient has the same bits from run to run with and
// without matgcn_set_deterministic.

struct HeadMcBwdArgs {
  const float* dS;       // (S, B, CH / od, N, od)
  const float* w;        // end_conv weight (CH, T, 64), plain
  const float* seq;      // step 0 of the T steps the head saw, time-major padded [T][B][Np][64]
  float* dSeq;           // the same steps of the sequence gradient
  float* wPart;          // [gridDim.x][CH][T][64]
  DropDesc drop;         // sample s draws with offset drop.offset + s
  int samples;
  int B, T, N, Np, CH, od;
};

constexpr int HMB_LD = 33;   // k_head_mc_wgrad: floats per node row of the staged tile (32 channels + 1: conflict-free writes)

// ---- the d_s tile of (b, n0 .. n0 + 31) in LDS -----------------------------------------------------------------------------
// thread tid fetches the elements idx = tid + 256 q (q < NQ) of the [rows][32] index space: row = channel, column = node
template <int NQ> struct HmbFetch { size_t ofs[NQ]; unsigned live; };
template <int NQ>
__device__ __forceinline__ HmbFetch<NQ> hmb_fetch_plan(const HeadMcBwdArgs& m, int b, int n0, int c0, int rows) {
  HmbFetch<NQ> f;
  f.live = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int idx = threadIdx.x + 256 * q, c = c0 + (idx >> 5), n = n0 + (idx & 31);
    f.ofs[q] = 0;
    if ((idx >> 5) < rows && c < m.CH && n < m.N) {
      const int o = c / m.od, dd = c - o * m.od;
      f.ofs[q] = (((size_t)b * (m.CH / m.od) + o) * m.N + n) * m.od + dd;
      f.live |= 1u << q;
    }
  }
  return f;
}
template <int NQ>
__device__ __forceinline__ void hmb_fetch(const HmbFetch<NQ>& f, const float* __restrict__ ds, float (&v)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) v[q] = (f.live >> q) & 1u ? ds[f.ofs[q]] : 0.f;
}

template <int K> struct HmbStep { static constexpr int value = K; };

// ---- dSeq ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head_mc_dseq(HeadMcBwdArgs m) {
  __shared__ float tile[2][64 * 32];      // [channel][node] of the sample being multiplied / the next one
  const int tilesPerB = (m.N + 31) >> 5;
  const int b = blockIdx.x / tilesPerB, n0 = (blockIdx.x % tilesPerB) * 32;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = lane & 31, half = lane >> 5;
  const int n = n0 + i;
  const int kPairs = (m.CH + 1) >> 1, rows = 2 * kPairs;   // an odd CH multiplies one row of zeros
  const size_t sampleFloats = (size_t)m.B * m.CH * m.N;
  const HmbFetch<8> plan = hmb_fetch_plan<8>(m, b, n0, 0, rows);
  f32x16 acc[6][2];
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int tl = 0; tl < 2; ++tl)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[k][tl][r] = 0.f;
  // mask quad of (b, step 0, n, hidden channels 4 half ..): a row past N decides nothing that is stored
  const unsigned long long qLane = ((unsigned long long)b * m.T * m.N + n) * 16 + half;
  float nx[8];
  hmb_fetch(plan, m.dS, nx);
  for (int s = 0; s < m.samples; ++s) {
    float* cur = tile[s & 1];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = threadIdx.x + 256 * q;
      if (idx < rows * 32) cur[idx] = nx[q];
    }
    if (s + 1 < m.samples) hmb_fetch(plan, m.dS + (size_t)(s + 1) * sampleFloats, nx);
    __syncthreads();
    DropDesc d = m.drop;
    d.offset += (unsigned long long)s;
    // the weight and the lane's mask position are the same for every sample: made opaque once per sample, or their loads
    // and the first Philox rounds of all steps are hoisted and kept live across the loop (see k_head_mc)
    const float* wbase = m.w;
    asm volatile("" : "+s"(wbase));
    unsigned int qlo = (unsigned int)qLane, qhi = (unsigned int)(qLane >> 32);
    asm volatile("" : "+v"(qlo), "+v"(qhi));
    const unsigned long long qb = ((unsigned long long)qhi << 32) | qlo;
    auto step = [&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      const int t = w + 4 * k;
      if (t < m.T) {   // wave-uniform
        f32x16 p[2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl)
#pragma unroll
          for (int r = 0; r < 16; ++r) p[tl][r] = 0.f;
        // A = W_t^T: lane (i, half) holds W[2 kk + half][t][32 tl + i]; B = the staged tile: d_s[2 kk + half][n0 + i]
        const float* wl = wbase + ((size_t)half * m.T + t) * 64 + i;
        const size_t wStride = (size_t)2 * m.T * 64;
#pragma nounroll
        for (int kk = 0; kk < kPairs; ++kk) {   // (rolled: the trip count is a run-time value and the body two dependent chains)
          const bool in = 2 * kk + half < m.CH;
          const float a0 = in ? wl[kk * wStride] : 0.f, a1 = in ? wl[kk * wStride + 32] : 0.f;
          const float bv = cur[(2 * kk + half) * 32 + i];
          p[0] = MFMA32(a0, bv, p[0]);
          p[1] = MFMA32(a1, bv, p[1]);
        }
        // accumulator rows 4 g .. 4 g + 3 of tile tl: hidden channels 32 tl + 8 g + 4 half .. + 3 of node n - one mask quad
        const unsigned long long q0 = qb + (unsigned long long)t * m.N * 16;
#pragma unroll
        for (int tl = 0; tl < 2; ++tl)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 mk = drop_mult4(d, q0 + 8 * tl + 2 * g);
            acc[k][tl][4 * g + 0] += mk.x * p[tl][4 * g + 0];
            acc[k][tl][4 * g + 1] += mk.y * p[tl][4 * g + 1];
            acc[k][tl][4 * g + 2] += mk.z * p[tl][4 * g + 2];
            acc[k][tl][4 * g + 3] += mk.w * p[tl][4 * g + 3];
          }
      }
    };
    step(HmbStep<0>{}); step(HmbStep<1>{}); step(HmbStep<2>{}); step(HmbStep<3>{}); step(HmbStep<4>{}); step(HmbStep<5>{});
  }
  if (n >= m.N) return;
  auto store = [&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    const int t = w + 4 * k;
    if (t < m.T) {
      float* dst = m.dSeq + (((size_t)t * m.B + b) * m.Np + n) * 64 + 4 * half;
#pragma unroll
      for (int tl = 0; tl < 2; ++tl)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(dst + 32 * tl + 8 * g) =
              make_float4(acc[k][tl][4 * g], acc[k][tl][4 * g + 1], acc[k][tl][4 * g + 2], acc[k][tl][4 * g + 3]);
    }
  };
  store(HmbStep<0>{}); store(HmbStep<1>{}); store(HmbStep<2>{}); store(HmbStep<3>{}); store(HmbStep<4>{}); store(HmbStep<5>{});
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
constexpr int HMB_WSTEPS = 3;    // steps per wave of k_head_mc_wgrad: a workgroup covers 12
__global__ __launch_bounds__(256) void k_head_mc_wgrad(HeadMcBwdArgs m) {
  __shared__ float tile[2][32 * HMB_LD];  // [node][channel] of the sample being multiplied / the next one
  const int tilesPerB = (m.N + 31) >> 5, items = m.B * tilesPerB;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = lane & 31, half = lane >> 5;
  const int c0 = blockIdx.z * 32, tBase = blockIdx.y * 4 * HMB_WSTEPS;
  const int quad = i >> 2, mq = i & 3;
  const size_t sampleFloats = (size_t)m.B * m.CH * m.N;
  f32x16 acc[HMB_WSTEPS][2];
#pragma unroll
  for (int k = 0; k < HMB_WSTEPS; ++k)
#pragma unroll
    for (int tl = 0; tl < 2; ++tl)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[k][tl][r] = 0.f;
  int buf = 0;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = item / tilesPerB, n0 = (item - b * tilesPerB) * 32;
    const HmbFetch<4> plan = hmb_fetch_plan<4>(m, b, n0, c0, 32);
    // B before the multipliers: lane (i, half) holds seq[b][t][n0 + 2 kk + half][32 tl + i]
    float sv[HMB_WSTEPS][2][16];
#pragma unroll
    for (int k = 0; k < HMB_WSTEPS; ++k) {
      const int t = tBase + w + 4 * k;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const int node = n0 + 2 * kk + half;
        const bool in = t < m.T && node < m.N;
        const float* rowp = m.seq + (((size_t)min(t, m.T - 1) * m.B + b) * m.Np + min(node, m.Np - 1)) * 64 + i;
        sv[k][0][kk] = in ? rowp[0] : 0.f;
        sv[k][1][kk] = in ? rowp[32] : 0.f;
      }
    }
    // mask quad of (b, step 0, node n0 + half, hidden channels 4 quad ..)
    const unsigned long long qLane = ((unsigned long long)b * m.T * m.N + n0 + half) * 16 + quad;
    float nx[4];
    hmb_fetch(plan, m.dS, nx);
    for (int s = 0; s < m.samples; ++s, buf ^= 1) {
      float* cur = tile[buf];
#pragma unroll
      for (int q = 0; q < 4; ++q) {       // 32 channels x 32 nodes: four elements per thread, stored node-major
        const int idx = threadIdx.x + 256 * q;
        cur[(idx & 31) * HMB_LD + (idx >> 5)] = nx[q];
      }
      if (s + 1 < m.samples) hmb_fetch(plan, m.dS + (size_t)(s + 1) * sampleFloats, nx);
      __syncthreads();
      DropDesc d = m.drop;
      d.offset += (unsigned long long)s;
      unsigned int qlo = (unsigned int)qLane, qhi = (unsigned int)(qLane >> 32);
      asm volatile("" : "+v"(qlo), "+v"(qhi));
      const unsigned long long qb = ((unsigned long long)qhi << 32) | qlo;
      // A = d_s^T: lane (i, half) holds d_s[c0 + i][n0 + 2 kk + half]
      float av[16];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) av[kk] = cur[(2 * kk + half) * HMB_LD + i];
      auto step = [&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        const int t = tBase + w + 4 * k;
        if (t < m.T) {   // wave-uniform
          const unsigned long long q0 = qb + (unsigned long long)t * m.N * 16;
#pragma unroll
          for (int tl = 0; tl < 2; ++tl) {
            // lane mq of a quad draws the mask quads of the node pairs kk = mq + 4 u: bits 4 u .. 4 u + 3
            unsigned int mine = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
              mine |= drop_keep4(d, q0 + (unsigned long long)(2 * (mq + 4 * u)) * 16 + 8 * tl) << (4 * u);
            unsigned int pk[4];
#pragma unroll
            for (int src = 0; src < 4; ++src) pk[src] = __shfl(mine, (lane & ~3) | src, 64);
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
              const bool kept = (pk[kk & 3] >> (4 * (kk >> 2) + mq)) & 1u;
              const float bv = kept ? sv[k][tl][kk] * d.scale : 0.f;
              acc[k][tl] = MFMA32(av[kk], bv, acc[k][tl]);
            }
          }
        }
      };
      static_assert(HMB_WSTEPS == 3, "one call per step below");
      step(HmbStep<0>{}); step(HmbStep<1>{}); step(HmbStep<2>{});
    }
  }
  // rows = channels c0 + acc_row(r, half), columns = hidden channels 32 tl + i
  float* part = m.wPart + (size_t)blockIdx.x * m.CH * m.T * 64;
  auto store = [&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    const int t = tBase + w + 4 * k;
    if (t < m.T) {
#pragma unroll
      for (int tl = 0; tl < 2; ++tl)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = c0 + acc_row(r, half);
          if (c < m.CH) part[((size_t)c * m.T + t) * 64 + 32 * tl + i] = acc[k][tl][r];
        }
    }
  };
  store(HmbStep<0>{}); store(HmbStep<1>{}); store(HmbStep<2>{});
}

// ---- bias gradient: block (c, s) adds d_s[., c, .] in a fixed order, one thread per channel then adds the samples ------------
__global__ __launch_bounds__(256) void k_head_mc_dbias_partial(HeadMcBwdArgs m, double* __restrict__ part) {
  __shared__ double red[4];
  const int c = blockIdx.x, s = blockIdx.y, o = c / m.od, dd = c - o * m.od;
  const float* src = m.dS + (size_t)s * m.B * m.CH * m.N;
  const int total = m.B * m.N;
  double v = 0.0;
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int b = idx / m.N, n = idx - b * m.N;
    v += (double)src[(((size_t)b * (m.CH / m.od) + o) * m.N + n) * m.od + dd];
  }
  for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_down(v, sh, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)s * m.CH + c] = ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ __launch_bounds__(64) void k_head_mc_dbias_final(const double* __restrict__ part, int samples, int CH,
                                                            float* __restrict__ dBias) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= CH) return;
  double v = 0.0;
  for (int s = 0; s < samples; ++s) v += part[(size_t)s * CH + c];
  dBias[c] = (float)v;
}

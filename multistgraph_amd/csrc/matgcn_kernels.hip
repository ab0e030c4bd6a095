// matgcn_kernels.hip - hand-written gfx950 (CDNA4, wave64) kernels of the Multi-ATGCN forward path.
//
// Every kernel cites the reference lines (libcity/model/traffic_flow_prediction/MultiATGCN.py) whose
// arithmetic it implements.  All matrix contractions run on the exact-fp32 matrix cores:
//   v_mfma_f32_16x16x4_f32 (graph mix, node kernels): lane l supplies A[row = l&15][k = l>>4], B[k = l>>4][col = l&15];
//     its 4 accumulator registers hold C[row = 4*(l>>4) + e][col = l&15];
//   v_mfma_f32_32x32x2_f32 (output head): A[row = l&31][k = l>>5], B[k = l>>5][col = l&31];
//     its 16 accumulator registers hold C[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31].
// This file: support stack, weight-stream preparation, layout helpers, head fusion, the graph-mix GEMM, the output
// head and the loss epilogue; the node-wise step kernels live in matgcn_node16.hip (same translation unit).
//
// Data layout (all fp32, Np = N rounded up to 16, H = 64; DESIGN.md section 3 has the full tables):
//   St   [Np][Mp]              transposed dense support stack, column k*Np+n holds S_k[n][.]   (mix A operand)
//   StT  [Np][rup(Ks*N,64)]    its tight copy, column k*N+n (written with St: k_adaptive_stack / k_static_stack; k_stack_tight on
//                              the Chebyshev and cheb_order = 1 paths)   (A operand of the forward's fp32 64 x 64 mix)
//   Hx   [rows][Np][64]        recurrent state / any per-row node features                    (mix B operand)
//   G    [N][rows][Ks][64]     graph-mixed features, node-major                                (node GEMM A operand)
//   W*   [N][K/16][OT][64][4]  node-adaptive weights in 16x16x4 B-fragment order               (node GEMM B operand)
//   PX   [T][N][B][192]        hoisted x-part of gate|update pre-activations (+bias), layers >= 1
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "matgcn_internal.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((ext_vector_type(4))) float f32x4;
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// =================================================================================================
// 1. support stack
// =================================================================================================
// Adaptive adjacency, one workgroup per row n (MultiATGCN.py:80-83):
//   A[n][m] = softmax_m(relu(sum_r E1[n][r] * E2[r][m]))      (unidirection)
//   A[n][m] = softmax_m(relu(sum_d E[n][d]  * E[m][d]))       (bidirection)
// Every logit is computed ONCE (kept in LDS: `lds` holds N floats) and the row is written contiguously into the plain
// matrix P[n][ldP]; k_static_transpose then moves it into its transposed stack slot with tiled, coalesced accesses
// (round 1 recomputed the logits in all three softmax passes and scattered 4-byte stores down a column of St).
__global__ __launch_bounds__(256) void k_adaptive_adj(const float* __restrict__ e1, const float* __restrict__ e2,
                                                      int rank, int bidir, int N, float* __restrict__ plain, int ldP) {
  extern __shared__ float logits[];      // N floats
  __shared__ float red[256];
  __shared__ float erow[64];
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int r = tid; r < rank; r += 256) erow[r] = e1[(size_t)n * rank + r];
  __syncthreads();
  float mx = 0.f;  // relu output is >= 0
  for (int m = tid; m < N; m += 256) {
    float s = 0.f;
    if (bidir) {
      for (int r = 0; r < rank; ++r) s = fmaf(erow[r], e1[(size_t)m * rank + r], s);
    } else {
      for (int r = 0; r < rank; ++r) s = fmaf(erow[r], e2[(size_t)r * N + m], s);
    }
    s = fmaxf(s, 0.f);
    logits[m] = s;
    mx = fmaxf(mx, s);
  }
  red[tid] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
  float sum = 0.f;
  for (int m = tid; m < N; m += 256) {
    const float e = expf(logits[m] - mx);
    logits[m] = e;
    sum += e;
  }
  red[tid] = sum;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const float inv = 1.0f / red[0];
  for (int m = tid; m < N; m += 256) plain[(size_t)n * ldP + m] = logits[m] * inv;
}

// static first-order supports (model.supports[s][1], MultiATGCN.py:269-283) -> transposed slots
// (accumulate: add into the slot instead - cheb_order = 1 sums its dense supports, see StackMap)
// (ldSrc: leading dimension of S - N for the reference's supports, the plain buffer's pitch for the adaptive adjacency)
__global__ __launch_bounds__(256) void k_static_transpose(const float* __restrict__ S, int N, int ldSrc,
                                                          float* __restrict__ St, int ldS, int col0,
                                                          float* __restrict__ plain, int ldP, int accumulate) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;  // bx: m block, by: n block
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int n = by + j, m = bx + tx;
    const float v = (n < N && m < N) ? S[(size_t)n * ldSrc + m] : 0.f;
    tile[j][tx] = v;
    if (plain && plain != S && n < N && m < N) plain[(size_t)n * ldP + m] = v;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int m = bx + j, n = by + tx;
    if (m < N && n < N) {
      float* dst = &St[(size_t)m * ldS + col0 + n];
      *dst = accumulate ? *dst + tile[tx][j] : tile[tx][j];
    }
  }
}

// Chebyshev recursion T_k = 2 S T_{k-1} - T_{k-2} (MultiATGCN.py:98-99): prod = S T_{k-1} comes from k_mix
// (plain output); this kernel forms T_k, stores it transposed into its stack slot and plain for the next order.
__global__ __launch_bounds__(256) void k_cheb_combine(const float* __restrict__ prod, const float* __restrict__ prev2,
                                                      int prev2_is_identity, int N, int ldP, float* __restrict__ St,
                                                      int ldS, int col0, float* __restrict__ plain_out) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    const int n = by + j, m = bx + tx;
    float v = 0.f;
    if (n < N && m < N) {
      const float p2 = prev2_is_identity ? (n == m ? 1.f : 0.f) : prev2[(size_t)n * ldP + m];
      v = 2.0f * prod[(size_t)n * ldP + m] - p2;
      plain_out[(size_t)n * ldP + m] = v;
    }
    tile[j][tx] = v;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int m = bx + j, n = by + tx;
    if (m < N && n < N) St[(size_t)m * ldS + col0 + n] = tile[tx][j];
  }
}

// The finished stack St [Np][ldS] (column k*Np + n) -> its tight copy [Np][ldT] (column k*N + n, zero from Ks*N on):
// the A operand of the forward's fp32 64 x 64 mixes (k_mix), which then launch over Ks*N stacked rows.  Writes every
// element of the copy; once per matgcn_prepare.
__global__ __launch_bounds__(256) void k_stack_tight(const float* __restrict__ St, int ldS, int Np, int N, int Ks,
                                                     float* __restrict__ tight, int ldT) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)Np * ldT) return;
  const int m = (int)(idx / ldT), c = (int)(idx % ldT);
  const int k = c / N, n = c - k * N;
  tight[idx] = k < Ks ? St[(size_t)m * ldS + k * Np + n] : 0.f;
}

// ---- cheb_k == 2 without sumDense: both stacks in at most two launches, no memset, no staging matrix ----
// Every dense first-order support owns exactly one slot, so a support can be stored straight into its columns of St
// (column k*Np + n) and of the tight copy StT (column k*N + n).  k_adaptive_stack writes slot 0 (the adaptive support is
// always the first dense one), k_static_stack every other slot, and together they write EVERY element of both buffers:
// rows m >= N and the columns n >= N of a slot as zeros, and - the launch that is told so (`tail`) - the columns behind
// the last slot (St: Ks*Np .. ldS, StT: Ks*N .. ldT).  `prepared` may hold anything before.
__device__ __forceinline__ void stack_tail_zero(float* __restrict__ St, int ldS, float* __restrict__ StT, int ldT,
                                                int Np, int N, int Ks, int block, int nBlocks, int tid, int nThreads) {
  const int s0 = Ks * Np, t0 = Ks * N, ws = ldS - s0, wt = ldT - t0;
  for (int m = block; m < Np; m += nBlocks) {
    for (int c = tid; c < ws; c += nThreads) St[(size_t)m * ldS + s0 + c] = 0.f;
    for (int c = tid; c < wt; c += nThreads) StT[(size_t)m * ldT + t0 + c] = 0.f;
  }
}

// The row softmax of k_adaptive_adj, value for value (same partition of a row over 256 threads, same reduction trees,
// same expf, maximum and division), for ROWS rows per workgroup - one group of 256 threads each - so that the transposed
// store moves ROWS consecutive columns per row m: 16 bytes at ROWS = 4 (ROWS = 1: graphs whose four rows of logits
// would not fit the LDS).  grid = Np / ROWS (Np is a multiple of 16); dynamic LDS = ROWS * N floats.
template <int ROWS>
__global__ __launch_bounds__(256 * ROWS) void k_adaptive_stack(const float* __restrict__ e1, const float* __restrict__ e2,
                                                               int rank, int bidir, int N, int Np, int Ks,
                                                               float* __restrict__ St, int ldS, float* __restrict__ StT,
                                                               int ldT, int tail) {
  extern __shared__ float logitsAll[];   // ROWS x N floats
  __shared__ float redAll[ROWS][256];
  __shared__ float erowAll[ROWS][64];
  __shared__ float invAll[ROWS];
  const int sub = threadIdx.x >> 8, tid = threadIdx.x & 255;
  const int n0 = blockIdx.x * ROWS, n = n0 + sub;
  const bool live = n < N;                 // a padding column: zeros, but every barrier is still met
  float* logits = logitsAll + (size_t)sub * N;
  float* red = redAll[sub];
  float* erow = erowAll[sub];
  if (live)
    for (int r = tid; r < rank; r += 256) erow[r] = e1[(size_t)n * rank + r];
  __syncthreads();
  float mx = 0.f;  // relu output is >= 0
  if (live)
    for (int m = tid; m < N; m += 256) {
      float s = 0.f;
      if (bidir) {
        for (int r = 0; r < rank; ++r) s = fmaf(erow[r], e1[(size_t)m * rank + r], s);
      } else {
        for (int r = 0; r < rank; ++r) s = fmaf(erow[r], e2[(size_t)r * N + m], s);
      }
      s = fmaxf(s, 0.f);
      logits[m] = s;
      mx = fmaxf(mx, s);
    }
  red[tid] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
  float sum = 0.f;
  if (live)
    for (int m = tid; m < N; m += 256) {
      const float e = expf(logits[m] - mx);
      logits[m] = e;
      sum += e;
    }
  red[tid] = sum;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) invAll[sub] = 1.0f / red[0];
  __syncthreads();
  // transposed store: row m of both stacks takes columns n0 .. n0 + ROWS - 1 of slot 0
  for (int m = threadIdx.x; m < Np; m += 256 * ROWS) {
    float v[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) v[j] = (m < N && n0 + j < N) ? logitsAll[(size_t)j * N + m] * invAll[j] : 0.f;
    float* ds = St + (size_t)m * ldS + n0;       // n0 + ROWS <= Np: inside the slot
    float* dt = StT + (size_t)m * ldT + n0;      // columns < N only: column N is the next support's first
    if (ROWS == 4) {
      *reinterpret_cast<float4*>(ds) = make_float4(v[0], v[1], v[2], v[3]);
      if (n0 + 4 <= N) *reinterpret_cast<float4*>(dt) = make_float4(v[0], v[1], v[2], v[3]);
      else
#pragma unroll
        for (int j = 0; j < ROWS; ++j) if (n0 + j < N) dt[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < ROWS; ++j) {
        ds[j] = v[j];
        if (n0 + j < N) dt[j] = v[j];
      }
    }
  }
  if (tail) stack_tail_zero(St, ldS, StT, ldT, Np, N, Ks, blockIdx.x, gridDim.x, threadIdx.x, 256 * ROWS);
}

// every static dense support -> its slot of both stacks: blockIdx.z picks the support, a workgroup turns one 32 x 32
// tile through LDS as k_static_transpose does and covers the Np x Np extent of the slot
struct StaticStackArgs {
  const float* S[4];     // (N, N) supports
  int slot[4];           // stack slot of each
};
__global__ __launch_bounds__(256) void k_static_stack(StaticStackArgs a, int N, int Np, int Ks, float* __restrict__ St,
                                                      int ldS, float* __restrict__ StT, int ldT, int tail) {
  __shared__ float tile[32][33];
  const float* __restrict__ S = a.S[blockIdx.z];
  const int slot = a.slot[blockIdx.z];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;  // bx: m block, by: n block
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int n = by + j, m = bx + tx;
    tile[j][tx] = (n < N && m < N) ? S[(size_t)n * N + m] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int m = bx + j, n = by + tx;
    if (m < Np && n < Np) {
      St[(size_t)m * ldS + slot * Np + n] = tile[tx][j];
      if (n < N) StT[(size_t)m * ldT + slot * N + n] = tile[tx][j];
    }
  }
  if (tail)
    stack_tail_zero(St, ldS, StT, ldT, Np, N, Ks, (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x),
                    (int)(gridDim.x * gridDim.y * gridDim.z), threadIdx.x, 256);
}

// =================================================================================================
// 2. node-adaptive weights in MFMA fragment order
// =================================================================================================
// W[n][k][i][o] = g_k * sum_d E[n][d] * Wpool[d][k][i][o], bias[n][o] = sum_d E[n][d] * bpool[d][o]
// (MultiATGCN.py:102-105; g = softmax(weights_g) is folded here instead of scaling the stack; diagonal supports
// are folded into the identity slot, see StackMap).  One thread produces, for PREP_NB consecutive nodes, the
// float4 a lane feeds to 4 consecutive MFMAs, so every pool element it reads serves PREP_NB nodes.
#define PREP_NB 8

// Chebyshev value t_order(s): t_0 = 1, t_1 = s, t_j = 2 s t_{j-1} - t_{j-2}   (MultiATGCN.py:98-99 on a diagonal)
__device__ __forceinline__ float cheb_scalar(float s, int order) {
  float t0 = 1.f, t1 = s;
  for (int j = 2; j <= order; ++j) { const float t2 = 2.f * s * t1 - t0; t0 = t1; t1 = t2; }
  return t1;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_prep_stream(PrepStream a) {
  const int nBase = blockIdx.y * PREP_NB;
  const int unit = blockIdx.x * 256 + threadIdx.x;
  const int OT = a.O >> 4;
  if (unit >= a.groups * OT * 64) return;
  const int lane = unit & 63, ct = (unit >> 6) % OT, g = (unit >> 6) / OT;
  const int o = 16 * ct + (lane & 15);
  // decode the 4 rows of this lane's float4
  int slot[4], chan[4];   // kept slot (-1: zero row, -2: bias row) and input channel
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (KIND == 0) {
      const int kk = 16 * g + 4 * (lane >> 4) + s;
      slot[s] = kk >> 6; chan[s] = a.iOfs + (kk & 63);
    } else if (KIND == 1) {
      const int kk = 16 * g + 4 * (lane >> 4) + s;
      const int nx = a.map.nKeep * a.C0;
      if (kk < nx) { slot[s] = kk / a.C0; chan[s] = kk - slot[s] * a.C0; }
      else { slot[s] = kk == nx ? -2 : -1; chan[s] = 0; }
    }
  }
  // softmax over the stack weights (tiny)
  float gmax = -3.0e38f, gsum = 1.f;
  if (a.wg) {
    gsum = 0.f;
    for (int k = 0; k < a.map.KtotOrig; ++k) gmax = fmaxf(gmax, a.wg[k]);
    for (int k = 0; k < a.map.KtotOrig; ++k) gsum += expf(a.wg[k] - gmax);
  }
  auto gk = [&](int k) { return a.wg ? expf(a.wg[k] - gmax) / gsum : 1.f; };
  const size_t dstride = (size_t)a.map.KtotOrig * a.I * a.O;
  float acc[PREP_NB][4];
#pragma unroll
  for (int b = 0; b < PREP_NB; ++b)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[b][s] = 0.f;
  // kept slots (and the bias row): one pool offset per row
  size_t rofs[4];
  float scale[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    rofs[s] = 0; scale[s] = 0.f;
    if (slot[s] >= 0) {
      const int k = a.map.keepK[slot[s]];
      rofs[s] = ((size_t)k * a.I + chan[s]) * a.O + o;
      scale[s] = gk(k);
    } else if (slot[s] == -2) {
      scale[s] = 1.f;
    }
  }
#pragma unroll 4
  for (int dd = 0; dd < a.d; ++dd) {
    float pv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float v = 0.f;
      if (slot[s] >= 0) v = a.wpool[(size_t)dd * dstride + rofs[s]];
      else if (slot[s] == -2) v = a.bpool[(size_t)dd * a.O + o];
      pv[s] = v * scale[s];
    }
#pragma unroll
    for (int b = 0; b < PREP_NB; ++b) {
      const float e = a.E[(size_t)min(nBase + b, a.N - 1) * a.d + dd];
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[b][s] = fmaf(e, pv[s], acc[b][s]);
    }
  }
  // folded diagonal supports: identity-slot rows also take t_order(s_n) * g_k * W[n][k]
  const bool anyIdent = slot[0] == 0 || slot[1] == 0 || slot[2] == 0 || slot[3] == 0;
  if (anyIdent) {
    for (int q = 0; q < a.map.nDiag; ++q) {
      const int k = a.map.diagK[q];
      const float gq = gk(k);
      float part[PREP_NB][4];
#pragma unroll
      for (int b = 0; b < PREP_NB; ++b)
#pragma unroll
        for (int s = 0; s < 4; ++s) part[b][s] = 0.f;
      for (int dd = 0; dd < a.d; ++dd) {
        float pv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
          pv[s] = slot[s] == 0 ? a.wpool[(size_t)dd * dstride + ((size_t)k * a.I + chan[s]) * a.O + o] : 0.f;
#pragma unroll
        for (int b = 0; b < PREP_NB; ++b) {
          const float e = a.E[(size_t)min(nBase + b, a.N - 1) * a.d + dd];
#pragma unroll
          for (int s = 0; s < 4; ++s) part[b][s] = fmaf(e, pv[s], part[b][s]);
        }
      }
#pragma unroll
      for (int b = 0; b < PREP_NB; ++b) {
        const int n = min(nBase + b, a.N - 1);
        const float t = gq * cheb_scalar(a.map.diagSrc[q][(size_t)n * (a.map.N + 1)], a.map.diagOrder[q]);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[b][s] = fmaf(t, part[b][s], acc[b][s]);
      }
    }
  }
  size_t frag;
  if (a.OTdst > 0) frag = ((size_t)(g * a.OTdst + a.otOfs + ct) * 64 + lane) * 4;
  else frag = (size_t)unit * 4;
#pragma unroll
  for (int b = 0; b < PREP_NB; ++b) {
    const int n = nBase + b;
    if (n < a.N)
      *reinterpret_cast<float4*>(a.out + (size_t)n * a.nodeStride + a.baseOfs + frag) =
          make_float4(acc[b][0], acc[b][1], acc[b][2], acc[b][3]);
  }
}

// Round 3: the same streams on the matrix cores.  W[n][row][o] = sum_d pool[d][row][o] * E[n][d] is a GEMM with the embedding
// dimension as its (short) reduction: A = 16 pool elements x d, B = d x 16 nodes, and the 16 A rows are chosen so that
// the accumulator of a lane - rows 4 (l >> 4) + e, column l & 15 of the 16x16x4 fp32 MFMA - is exactly one float4 of the
// fragment stream of node l & 15: rows 4 q + s of a "quad" are the four weight rows s of the float4 in slot j = 4 j4 + q
// of lane group kq.  A wave keeps the A fragments of 8 quads (half a fragment row: 2 lane groups x 4 j4) in registers and
// walks 16-node tiles; per tile it reads 4 ceil(d / 4) embedding values, issues 8 ceil(d / 4) MFMAs and stores 8 float4
// per lane (64-byte pieces that the L2 merges into the node's 1 KB rows).  The exact-fp32 MFMA accumulates k = 0..3 in
// order, so the sums are the fma chains of the kernel above.  DS = ceil(d / 4) steps are compiled in (3 / 5 / 8:
// embeddings of up to 12 / 20 / 32; wider ones take the first kernel).  `groups` k-groups of kind-0 rows are followed by
// `groupsX` k-groups of kind-1 rows (layer 0: the folded x rows and the bias row sit behind the recurrent rows of the same
// node stream, so one launch writes both).  Measured at N = 403, d = 20 (profiles/r03_prep_lab.log): 27 us per launch
// against 49 us (+ 35 us for the kind-1 launch) of the first kernel, which re-reads every pool value per 8 nodes and
// spends 2 d VALU fmas per output; a VALU variant with the pool values in registers and a node loop was slower (68 us).
template <int DS>
__global__ __launch_bounds__(256) void k_prep_mfma(PrepStream a, int tilesPerBlock) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int OT = a.O >> 4;
  const int pair = blockIdx.x >> 1, half = blockIdx.x & 1;
  const int ct = pair % OT, g = pair / OT;
  const int r = lane & 15, ka = lane >> 4;      // A operand: row r of the quad (slot r >> 2, weight row s = r & 3), d index ka
  float gmax = -3.0e38f, gsum = 1.f;
  if (a.wg) {
    gsum = 0.f;
    for (int k = 0; k < a.map.KtotOrig; ++k) gmax = fmaxf(gmax, a.wg[k]);
    for (int k = 0; k < a.map.KtotOrig; ++k) gsum += expf(a.wg[k] - gmax);
  }
  auto gk = [&](int k) { return a.wg ? expf(a.wg[k] - gmax) / gsum : 1.f; };
  const size_t dstride = (size_t)a.map.KtotOrig * a.I * a.O;
  float A[8][DS], Aq[8][DS];
  bool ident = false;
#pragma unroll
  for (int q8 = 0; q8 < 8; ++q8) {
    const int kq = 2 * half + (q8 >> 2), j = 4 * (q8 & 3) + (r >> 2), sr = r & 3;
    const int o = 16 * ct + j;
    int slot, chan;
    if (g < a.groups) {
      const int kk = 16 * g + 4 * kq + sr;
      slot = kk >> 6; chan = a.iOfs + (kk & 63);
    } else {
      const int kk = 16 * (g - a.groups) + 4 * kq + sr;
      const int nx = a.map.nKeep * a.C0;
      if (kk < nx) { slot = kk / a.C0; chan = kk - slot * a.C0; }
      else { slot = kk == nx ? -2 : -1; chan = 0; }
    }
    const float* src = a.wpool; size_t sstep = 0; float scale = 0.f;
    if (slot >= 0) {
      const int k = a.map.keepK[slot];
      src = a.wpool + ((size_t)k * a.I + chan) * a.O + o; sstep = dstride; scale = gk(k);
    } else if (slot == -2) {
      src = a.bpool + o; sstep = (size_t)a.O; scale = 1.f;
    }
    const bool id = slot == 0 && a.map.nDiag > 0;
    ident = ident || id;
    const float* srcq = id ? a.wpool + ((size_t)a.map.diagK[0] * a.I + chan) * a.O + o : a.wpool;
#pragma unroll
    for (int st = 0; st < DS; ++st) {
      const int dd = 4 * st + ka;
      const float v = src[(size_t)min(dd, a.d - 1) * sstep];
      A[q8][st] = (dd < a.d && slot != -1) ? v * scale : 0.f;
      const float vq = srcq[(size_t)min(dd, a.d - 1) * (id ? dstride : 0)];
      Aq[q8][st] = (dd < a.d && id) ? vq : 0.f;
    }
  }
  const bool anyIdent = __ballot(ident) != 0ull;
  const int nTiles = (a.N + 15) >> 4;
  const int tile0 = blockIdx.y * tilesPerBlock, tile1 = min(tile0 + tilesPerBlock, nTiles);
  const int nodeL = lane & 15, kb = lane >> 4;   // B operand / accumulator: node of the tile, d index; slot quarter kb
  auto load_b = [&](int tile, float (&Bf)[DS]) {
    const float* e = a.E + (size_t)min(tile * 16 + nodeL, a.N - 1) * a.d;
#pragma unroll
    for (int st = 0; st < DS; ++st) {
      const int dd = 4 * st + kb;
      const float v = e[min(dd, a.d - 1)];
      Bf[st] = dd < a.d ? v : 0.f;
    }
  };
  float Bf[DS], Bn[DS];
  if (tile0 + w < tile1) load_b(tile0 + w, Bf);
  for (int tile = tile0 + w; tile < tile1; tile += 4) {
    load_b(min(tile + 4, tile1 - 1), Bn);
    const int n = tile * 16 + nodeL;
    f32x4 acc[8];
#pragma unroll
    for (int q8 = 0; q8 < 8; ++q8) acc[q8] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < DS; ++st)
#pragma unroll
      for (int q8 = 0; q8 < 8; ++q8) acc[q8] = MFMA16(A[q8][st], Bf[st], acc[q8]);
    if (anyIdent) {
      const int nc = min(n, a.N - 1);
      for (int q = 0; q < a.map.nDiag; ++q) {
        f32x4 part[8];
#pragma unroll
        for (int q8 = 0; q8 < 8; ++q8) part[q8] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q == 0) {
#pragma unroll
          for (int st = 0; st < DS; ++st)
#pragma unroll
            for (int q8 = 0; q8 < 8; ++q8) part[q8] = MFMA16(Aq[q8][st], Bf[st], part[q8]);
        } else {   // further diagonal supports: their pool values are re-read (rare)
          const int k = a.map.diagK[q];
#pragma unroll
          for (int q8 = 0; q8 < 8; ++q8) {
            const int kq = 2 * half + (q8 >> 2), j = 4 * (q8 & 3) + (r >> 2), sr = r & 3;
            int slot, chan;
            if (g < a.groups) { const int kk = 16 * g + 4 * kq + sr; slot = kk >> 6; chan = a.iOfs + (kk & 63); }
            else {
              const int kk = 16 * (g - a.groups) + 4 * kq + sr;
              if (kk < a.map.nKeep * a.C0) { slot = kk / a.C0; chan = kk - slot * a.C0; } else { slot = -1; chan = 0; }
            }
#pragma unroll
            for (int st = 0; st < DS; ++st) {
              const int dd = 4 * st + ka;
              const float v = a.wpool[(size_t)min(dd, a.d - 1) * dstride + ((size_t)k * a.I + chan) * a.O + 16 * ct + j];
              part[q8] = MFMA16((dd < a.d && slot == 0) ? v : 0.f, Bf[st], part[q8]);
            }
          }
        }
        const float t = gk(a.map.diagK[q]) *
                        cheb_scalar(a.map.diagSrc[q][(size_t)nc * (a.map.N + 1)], a.map.diagOrder[q]);
#pragma unroll
        for (int q8 = 0; q8 < 8; ++q8)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[q8][e] = fmaf(t, part[q8][e], acc[q8][e]);
      }
    }
    if (n < a.N) {
      float* dst = a.out + (size_t)n * a.nodeStride + a.baseOfs;
#pragma unroll
      for (int q8 = 0; q8 < 8; ++q8) {
        const int kq = 2 * half + (q8 >> 2), j = 4 * (q8 & 3) + kb;
        const size_t frag = ((size_t)(a.OTdst > 0 ? g * a.OTdst + a.otOfs + ct : g * OT + ct) * 64 + kq * 16 + j) * 4;
        *reinterpret_cast<float4*>(dst + frag) = make_float4(acc[q8][0], acc[q8][1], acc[q8][2], acc[q8][3]);
      }
    }
#pragma unroll
    for (int st = 0; st < DS; ++st) Bf[st] = Bn[st];
  }
}

// bias[n][colOfs + o] = E[n] . bpool[:, o]   (hoisted-PX layers)
__global__ __launch_bounds__(256) void k_prep_bias(const float* __restrict__ E, const float* __restrict__ bpool, int d,
                                                   int O, int N, float* __restrict__ out, int ldo, int colOfs) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * O) return;
  const int n = idx / O, o = idx - n * O;
  float s = 0.f;
  for (int dd = 0; dd < d; ++dd) s = fmaf(E[(size_t)n * d + dd], bpool[(size_t)dd * O + o], s);
  out[(size_t)n * ldo + colOfs + o] = s;
}

// nn.Linear / Conv2d weight (O, I) -> fragment order [jg][OT][64][4] of B[j][o] = W[o][in(j)].
// Rows j < Cpad map to input j (zero beyond C); rows j >= Cpad map to input C + (j - Cpad).
// (one matrix of k_prep_dense, matgcn_node16.hip: `unit` is the float4 this thread writes)
__device__ __forceinline__ void prep_linear(const float* __restrict__ W, int I, int O, int C, int Cpad, int rows, int OT,
                                            float* __restrict__ out, int unit) {
  const int units = (rows >> 3) * OT * 64;
  if (unit >= units) return;
  const int lane = unit & 63, ot = (unit >> 6) % OT, jg = (unit >> 6) / OT;
  const int o = ot * 32 + (lane & 31);
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = jg * 8 + 4 * (lane >> 5) + q;
    int in = -1;
    if (j < Cpad) { if (j < C) in = j; } else { in = C + (j - Cpad); }
    v[q] = (in >= 0 && in < I && o < O) ? W[(size_t)o * I + in] : 0.f;
  }
  *reinterpret_cast<float4*>(out + (size_t)unit * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

// =================================================================================================
// 3. layout helpers (all tiny, HBM-trivial)
// =================================================================================================
// user (rows, N, C) -> padded [rows][Np][C] (pad rows zero)
__global__ __launch_bounds__(256) void k_pack_rows(const float* __restrict__ src, float* __restrict__ dst, int rows,
                                                   int N, int Np, int C) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)rows * Np * C;
  if (idx >= total) return;
  const int c = idx % C;
  const int n = (idx / C) % Np;
  const size_t r = idx / ((size_t)C * Np);
  dst[idx] = (src && n < N) ? src[(r * N + n) * C + c] : 0.f;
}

__global__ __launch_bounds__(256) void k_unpack_rows(const float* __restrict__ src, float* __restrict__ dst, int rows,
                                                     int N, int Np, int C) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)rows * N * C;
  if (idx >= total) return;
  const int c = idx % C;
  const int n = (idx / C) % N;
  const size_t r = idx / ((size_t)C * N);
  dst[idx] = src[(r * Np + n) * C + c];
}

// user (B, T, N, C) <-> padded time-major [T][B][Np][C]
__global__ __launch_bounds__(256) void k_pack_seq_tm(const float* __restrict__ src, float* __restrict__ dst, int B,
                                                     int T, int N, int Np, int C) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)T * B * Np * C;
  if (idx >= total) return;
  const int c = idx % C;
  const int n = (idx / C) % Np;
  const int b = (idx / ((size_t)C * Np)) % B;
  const int t = idx / ((size_t)C * Np * B);
  dst[idx] = (n < N) ? src[(((size_t)b * T + t) * N + n) * C + c] : 0.f;
}

__global__ __launch_bounds__(256) void k_unpack_seq_tm(const float* __restrict__ src, float* __restrict__ dst, int B,
                                                       int T, int N, int Np, int C) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)B * T * N * C;
  if (idx >= total) return;
  const int c = idx % C;
  const int n = (idx / C) % N;
  const int t = (idx / ((size_t)C * N)) % T;
  const int b = idx / ((size_t)C * N * T);
  dst[idx] = src[(((size_t)t * B + b) * Np + n) * C + c];
}

// zero rows n in [N, Np) of a [rows][Np][C] buffer
__global__ __launch_bounds__(256) void k_zero_pad_rows(float* __restrict__ buf, int rows, int N, int Np, int C) {
  const int per = (Np - N) * C;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * per) return;
  const size_t r = idx / per;
  const int q = idx - r * per;
  buf[(r * Np + N) * C + q] = 0.f;
}

// the same for up to 8 buffers of one shape in ONE launch (blockIdx.y picks the buffer), 16 bytes per thread (C % 4 == 0):
// the backward opens with six of them in front of its first chain
struct PadRowBufs { float* p[8]; };
__global__ __launch_bounds__(256) void k_zero_pad_rows_multi(PadRowBufs bufs, int rows, int N, int Np, int C) {
  const int per4 = (Np - N) * C / 4;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * per4) return;
  const size_t r = idx / per4;
  const int q = (int)(idx - r * per4);
  *reinterpret_cast<float4*>(bufs.p[blockIdx.y] + (r * Np + N) * C + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// =================================================================================================
// 4. temporal-head fusion prologue (MultiATGCN.py:365-402)
// =================================================================================================
// x0[b][t][n][c<od]  = sum_h softmax(weight_tsg)[h] * X[b][begin_h + t][n][start+c] * weight_ts[h][t][n][c]
// x0[b][t][n][od+j]  = X[b][t][n][ext_src[j]]           (time of day / dynamic channels)
// Series mode: row label_start[b] + offset of the device-resident series.  The caller guarantees the range
// (include/matgcn.h); a violated contract must not fault the device, so the row is clamped into the series and the
// violation counted (matgcn_series_violations reads and clears the counter).
__device__ unsigned long long g_series_violations = 0;
__device__ __forceinline__ size_t series_row(long row, long steps) {
  if (row < 0 || row >= steps) {
    atomicAdd(&g_series_violations, 1ull);
    row = row < 0 ? 0 : steps - 1;
  }
  return (size_t)row;
}
// the label row of (b, o); in it the od label channels of node n, and channel c of them
// (label_ptr and label_at each spell the offset: written through the other, instructions move in k_loss_grad or k_group_walk)
__device__ __forceinline__ size_t label_row(const LabelView& v, size_t b, int o) {
  return v.labelStart ? series_row((long)v.labelStart[b] + o, v.ySteps) : b * v.ySteps + o;
}
__device__ __forceinline__ const float* label_ptr(const LabelView& v, size_t row, int n) {
  return v.y + (row * v.N + n) * v.yFeat + v.yStart;
}
__device__ __forceinline__ float label_at(const LabelView& v, size_t row, int n, int c) {
  return v.y[(row * v.N + n) * v.yFeat + v.yStart + c];
}

// x * sd + mu as two fp32 roundings, the way the reference's tensors de-scale.  hipcc would fuse the pair into one fma
// (the __fmul_rn / __fadd_rn of the HIP headers are plain operators and fuse as well): half an ulp of the product is a
// visible share of a label that de-scales to nearly 0, and of its |d / l| (MAPE).
__device__ __forceinline__ float scale_affine(float x, float sd, float mu) {
#pragma clang fp contract(off)
  const float t = x * sd;
  return t + mu;
}
// the affines of node n, each two fp32 roundings
__device__ __forceinline__ float descale_node(const NodeScale& sc, int n, float v) {
  if (sc.std) v = scale_affine(v, sc.std[sc.perNode ? n : 0], sc.mean[sc.perNode ? n : 0]);
  if (sc.std2) v = scale_affine(v, sc.std2[n], sc.mean2[n]);
  return v;
}

__global__ __launch_bounds__(256) void k_fuse_heads(FuseArgs a) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)a.B * a.T * a.Np;   // the padding rows n >= N too: they are written as zeros here
  if (idx >= total) return;
  const int n = idx % a.Np;
  const int t = (idx / a.Np) % a.T;
  const int b = idx / ((size_t)a.Np * a.T);
  if (n >= a.N) {
    float* pad = a.x0 + idx * a.C0;
    for (int c = 0; c < a.C0; ++c) pad[c] = 0.f;
    return;
  }
  float gmax = -3.0e38f, gsum = 0.f;
  for (int h = 0; h < a.nTs; ++h) gmax = fmaxf(gmax, a.tsg[h]);
  for (int h = 0; h < a.nTs; ++h) gsum += expf(a.tsg[h] - gmax);
  // row `step` of sample b: a window row, or - series mode - the series row at label start + rel[step]
  auto xrow = [&](int step) -> const float* {
    const size_t r = a.labelStart ? series_row((long)a.labelStart[b] + a.rel[step], a.seriesSteps)
                                  : (size_t)b * a.xSteps + step;
    return a.X + (r * a.N + n) * a.F;
  };
  float* dst = a.x0 + (((size_t)b * a.T + t) * a.Np + n) * a.C0;
  for (int c = 0; c < a.od; ++c) {
    float acc = 0.f;
    for (int h = 0; h < a.nHeads; ++h) {
      const float g = expf(a.tsg[h] - gmax) / gsum;
      const float xv = xrow(a.headBegin[h] + t)[a.startDim + c];
      const float wv = a.ts[h][((size_t)t * a.N + n) * a.od + c];
      acc += g * xv * wv;
    }
    dst[c] = acc;
  }
  for (int j = 0; j < a.C0 - a.od; ++j)
    dst[a.od + j] = xrow(t)[a.extSrc[j]];
}

// layer-0 encoder input as a plain matrix for the mix GEMM: X0m[m][(row*C0 + c)] = x0p[row][m][c]
__global__ __launch_bounds__(256) void k_x0_to_matrix(const float* __restrict__ x0p, float* __restrict__ X0m, int rows,
                                                      int Np, int C0, int ld) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)Np * ld;
  if (idx >= total) return;
  const int col = idx % ld;
  const int m = idx / ld;
  float v = 0.f;
  if (col < rows * C0) {
    const int row = col / C0, c = col - row * C0;
    v = x0p[((size_t)row * Np + m) * C0 + c];
  }
  X0m[idx] = v;
}

// folded x-part of the layer-0 node GEMM: XA0[t][n][b][Kx] = [x0 (k=0) | mix_k(x0), k<Ks | 1.0 | 0...]
// (the 1.0 column meets the bias row of the folded weights)
// Both sides move whole lines.  For one node n the sources are rows of two matrices - X0m[n][.] (the x0 columns, as
// k_x0_to_matrix laid them out) and MX0[k*Np + n][.] - whose column (b*T + t)*C0 + c is contiguous over (t, c) for one
// b; the destination XA0[t][n][b0 ..][0 .. Kx) is contiguous over (b, j) for one t.  A workgroup takes (n, bChunk
// samples, tChunk steps): it reads (Ks + 1) * bChunk runs of tChunk*C0 floats into LDS [k][b][t*C0 + c] and writes
// tChunk runs of bChunk*Kx floats with 16-byte stores (Kx is a multiple of 16).  bChunk / tChunk: fold_x0, from the
// LDS the tile takes.  grid = (N, ceil(B / bChunk), ceil(T / tChunk)); dynamic LDS = (Ks+1)*bChunk*tChunk*C0 floats.
__global__ __launch_bounds__(256) void k_build_xa0(const float* __restrict__ X0m, const float* __restrict__ MX0,
                                                   float* __restrict__ XA0, int B, int T, int N, int Np, int C0,
                                                   int Ks, int Kx, int ld, int bChunk, int tChunk) {
  extern __shared__ float xs[];
  const int n = blockIdx.x, b0 = blockIdx.y * bChunk, t0 = blockIdx.z * tChunk;
  const int nb = min(bChunk, B - b0), nt = min(tChunk, T - t0);
  const int run = nt * C0, perK = nb * run;
  for (int i = threadIdx.x; i < (Ks + 1) * perK; i += 256) {
    const int k = i / perK, r = i - k * perK;
    const int bb = r / run, q = r - bb * run;
    const float* src = k == 0 ? X0m + (size_t)n * ld : MX0 + ((size_t)(k - 1) * Np + n) * ld;
    xs[i] = src[((size_t)(b0 + bb) * T + t0) * C0 + q];
  }
  __syncthreads();
  const int nx = (Ks + 1) * C0, kx4 = Kx >> 2, perT = nb * kx4;
  for (int i = threadIdx.x; i < nt * perT; i += 256) {
    const int tt = i / perT, r = i - tt * perT;
    const int bb = r / kx4, j0 = 4 * (r - bb * kx4);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      v[e] = 0.f;
      if (j < nx) {
        const int k = j / C0, c = j - k * C0;
        v[e] = xs[(k * nb + bb) * run + tt * C0 + c];
      } else if (j == nx) v[e] = 1.0f;
    }
    float* dst = XA0 + (((size_t)(t0 + tt) * N + n) * B + b0) * Kx + 4 * (size_t)r;
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// state initialisation of every layer in ONE launch per forward (blockIdx.y = layer), 16 bytes per thread:
//   ZHx_l [B][Np][64] <- 0;  Hx_l [B][Np][64] <- h0_l (user layout (B, N, 64), padding rows zero) or zeros;
//   H0_l (training forward with h0: the copy the backward reads) <- the same;
//   Seq_l [B*T][Np][64]: rows n >= N <- 0 (the update kernels write the rows of the real nodes only).
// Thread idx < state4 takes a float4 of the three state buffers, the threads behind it one of the padding rows.
struct StateInitArgs {
  float* zhx[4];
  float* hx[4];
  float* h0dst[4];        // or null
  const float* h0[4];     // or null: zero state
  float* seq[4];
};
__global__ __launch_bounds__(256) void k_state_init(StateInitArgs a, int B, int rowsSeq, int N, int Np) {
  const int l = blockIdx.y;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t state4 = (size_t)B * Np * 16;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (idx < state4) {
    const int c4 = (int)(idx & 15);
    const int n = (int)((idx >> 4) % Np);
    const size_t r = (idx >> 4) / Np;
    float4 v = zero;
    if (a.h0[l] && n < N) {
      const float* src = a.h0[l] + (r * N + n) * 64 + 4 * c4;   // a caller's tensor: no alignment beyond its floats
      v = make_float4(src[0], src[1], src[2], src[3]);
    }
    reinterpret_cast<float4*>(a.zhx[l])[idx] = zero;
    reinterpret_cast<float4*>(a.hx[l])[idx] = v;
    if (a.h0dst[l]) reinterpret_cast<float4*>(a.h0dst[l])[idx] = v;
    return;
  }
  const int per4 = (Np - N) * 16;
  const size_t q = idx - state4;
  if (q >= (size_t)rowsSeq * per4) return;
  const size_t r = q / per4;
  const int e = (int)(q - r * per4);
  *reinterpret_cast<float4*>(a.seq[l] + (r * Np + N) * 64 + 4 * e) = zero;
}

// =================================================================================================
// 5. graph mix GEMM (MultiATGCN.py:106):  out[(k,n)][col] = sum_m S_k[n][m] * X[m][col]
// =================================================================================================
// 64 x 64 output tile per workgroup, 4 waves, each a 32x32 tile as 2x2 accumulators of the 16x16x4 MFMA; K-step 16 staged through
// LDS (double buffer, fed from registers that run two tiles ahead of the MFMAs; one barrier per step).  A = St (k-major, so the tile is 16 rows of
// 256 contiguous bytes), B = 64 feature columns of one state row (256-byte lines).
// ROLE only names the instantiation (0: pre-passes and Chebyshev products, 1: the recurrent step's mix of h / z*h),
// so that profilers list the roofline kernel - the per-step launch - on its own line.
// FLUSH (round 4): the accumulators are one fp32 fma chain over the WHOLE reduction - 4 096 links at N = 4 096, where the
// reference's own prediction sits 4.7e-7 from its float64 run and this kernel's single chain left the path at 1.2e-6
// (tests/golden/fp64_gap.npz; a blocked CPU sgemm sums K in blocks of a few hundred).  With FLUSH the chain is cut every
// MIX_FLUSH_TILES K-tiles (256 reduction indices): partial sums go to a second accumulator set.  Launched for nK > 64 only,
// so every graph of at most 1 024 nodes - the headline's 403 - keeps its kernel and its bits.
// (round 4, measured and rejected: rotating the wave priority with the K-tile index by dispatch round so that the five
//  workgroups of a CU leave together - they do, and every one is slower: 43.0 vs 41.3 us, profiles/r04_mix_stamps_lab.log)
constexpr int MIX_FLUSH_TILES = 16;

// Tile order of every mix kernel: workgroups that share an XCD (id % 8) sweep the row tiles of one column unit back to
// back, so St and that X slice stay in its L2.  A column unit is a column tile (k_mix, k_mix_bf16), half a tile
// (k_mix_c32) or a pair of tiles (k_mix_n32).
__device__ __forceinline__ void mix_tile_order(int id, int nColUnits, int nRowTiles, int& rowTile, int& colUnit) {
  if ((nColUnits & 7) == 0) {
    const int xcd = id & 7, j = id >> 3, cpx = nColUnits >> 3;
    rowTile = j % nRowTiles;
    colUnit = xcd * cpx + j / nRowTiles;
  } else {
    rowTile = id % nRowTiles;
    colUnit = id / nRowTiles;
  }
}

template <int ROLE, bool FLUSH = false>
__global__ __launch_bounds__(256) void k_mix(MixArgs a) {
  // (FLUSH costs 16 registers, 72 in all: seven workgroups per CU instead of eight, +3.7 % per launch at N = 4 096; forced
  //  into 64 registers the compiler spilled a pointer inside the K loop, +6.5 %: profiles/r04_mix_lab.log)
  __shared__ __attribute__((aligned(16))) float As[2][16 * 64];
  __shared__ __attribute__((aligned(16))) float Bs[2][16 * 64];
  int colTile, rowTile;
  mix_tile_order(blockIdx.x, a.nColTiles, a.nRowTiles, rowTile, colTile);
  const int row0 = rowTile * 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, j = lane & 15, kq = lane >> 4;
  const int kk = tid >> 4, sg = tid & 15;
  const int part = blockIdx.y;     // split reduction (MixArgs.parts): 0 unless the launch has a second grid dimension
  const float* ap = a.St + (size_t)part * a.aPartStride + (size_t)kk * a.ldS + row0 + sg * 4;
  const float* bp = a.X + (size_t)part * a.xPartStride + (size_t)colTile * a.xTileStride + (size_t)kk * a.ldX + sg * 4;
  // LDS image of a K-tile: row kk (one reduction index, 64 values) rotated by 16*(kk&3) floats, so that the four
  // k rows one 16x16x4 MFMA step reads (kq = 0..3) sit in four different bank quarters
  const int stPos = kk * 64 + (((sg + 4 * (kk & 3)) & 15) << 2);
  // K-tile t+1 waits in registers while tile t is multiplied, and tile t+2 is already requested: two register
  // sets alternate (the loop is unrolled by two so that they stay named registers), loads are unconditional
  // (clamped to the last tile) so the compiler keeps counting them instead of draining the queue at a branch
  const int last = a.nK - 1;
  auto ldA = [&](int t) { return *reinterpret_cast<const float4*>(ap + (size_t)min(t, last) * 16 * a.ldS); };
  auto ldB = [&](int t) { return *reinterpret_cast<const float4*>(bp + (size_t)min(t, last) * 16 * a.ldX); };
  // All six requests of the prologue leave BEFORE the first wait (round 4: at 48 registers the compiler had serialised
  // them to save two - load A0, wait, store, load B0, wait, store, and only then tiles 1 and 2: two exposed memory round
  // trips in front of every launch's first MFMA; the sched_barrier pins the order, the stores then wait with vmcnt(5) / (4))
  float4 ra0, rb0, ra1, rb1;
  {
    const float4 a0 = ldA(0), b0 = ldB(0);
    __builtin_amdgcn_sched_barrier(0);    // tile 0 first: its stores wait for the two OLDEST requests only
    ra0 = ldA(1); rb0 = ldB(1); ra1 = ldA(2); rb1 = ldB(2);
    __builtin_amdgcn_sched_barrier(0);
    *reinterpret_cast<float4*>(&As[0][stPos]) = a0;
    *reinterpret_cast<float4*>(&Bs[0][stPos]) = b0;
  }
  __syncthreads();
  // the wave's 32x32 output tile = 2x2 accumulators of v_mfma_f32_16x16x4_f32: 20 independent accumulator chains
  // per SIMD at 5 resident workgroups per CU, enough to keep the matrix pipe issuing back to back
  f32x4 acc[2][2], tot[FLUSH ? 2 : 1][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (FLUSH) tot[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  const int rotA0 = (wr * 32 + j + 16 * kq) & 63, rotA1 = (wr * 32 + 16 + j + 16 * kq) & 63;
  const int rotB0 = (wc * 32 + j + 16 * kq) & 63, rotB1 = (wc * 32 + 16 + j + 16 * kq) & 63;
  auto mma = [&](int cur) {
    const float* A = &As[cur][kq * 64];
    const float* Bm = &Bs[cur][kq * 64];
#pragma unroll
    for (int s = 0; s < 4; ++s) {      // reduction indices 4s + kq of this K-tile
      const float a0 = A[s * 256 + rotA0], a1 = A[s * 256 + rotA1];
      const float b0 = Bm[s * 256 + rotB0], b1 = Bm[s * 256 + rotB1];
      acc[0][0] = MFMA16(a0, b0, acc[0][0]);
      acc[0][1] = MFMA16(a0, b1, acc[0][1]);
      acc[1][0] = MFMA16(a1, b0, acc[1][0]);
      acc[1][1] = MFMA16(a1, b1, acc[1][1]);
    }
  };
  for (int it = 0; it < a.nK; it += 2) {
    mma(0);                                               // tile it
    *reinterpret_cast<float4*>(&As[1][stPos]) = ra0;      // tile it+1 (a clamped copy past the end: unused)
    *reinterpret_cast<float4*>(&Bs[1][stPos]) = rb0;
    ra0 = ldA(it + 3); rb0 = ldB(it + 3);
    __syncthreads();
    if (it + 1 < a.nK) {
      mma(1);                                             // tile it+1
      *reinterpret_cast<float4*>(&As[0][stPos]) = ra1;    // tile it+2
      *reinterpret_cast<float4*>(&Bs[0][stPos]) = rb1;
      ra1 = ldA(it + 4); rb1 = ldB(it + 4);
      __syncthreads();
    }
    if constexpr (FLUSH) {
      if (((it + 2) & (MIX_FLUSH_TILES - 1)) == 0) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) tot[p][q][e] += acc[p][q][e];
            acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
  }
  if constexpr (FLUSH) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[p][q][e] += tot[p][q][e];
  }
  // Epilogue: each wave turns its 32x32 accumulator tile through LDS (the K-loop buffers are free after the last
  // barrier; 16-byte slots XOR-swizzled by row so both the scalar writes and the b128 reads are conflict-free)
  // and writes whole 128-byte row segments with 16-byte WRITE-THROUGH stores (sc1): the 20-75 MB this kernel
  // produces then leave the L2 while it is still computing instead of as one dirty-line flush at its end, which
  // the next kernel of the chain would otherwise wait for.
  // (round 4: the last workgroup of a CU runs this stretch alone, one wave per SIMD - 8.5 k cycles by the stamps of
  //  70c9db4:tools/labs/stamps_mix_r04.py: sixteen scalar LDS writes with seven address instructions each, then four
  //  times read -> wait -> 64-bit divide -> guarded store.  Now the sixteen offsets are three adds from precomputed pieces, the four
  //  rows are read in one batch, and a row outside the output is dropped by the buffer's range check instead of a branch.)
  float* stg = (w < 2 ? &As[0][0] : &Bs[0][0]) + (w & 1) * 1024;
  {
    const int jq = j >> 2, jr = j & 3, kb = kq & 1;
    int xe[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) xe[e] = e * 32 + ((jq ^ e) << 2) + jr;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int base = (p * 16 + 4 * kq) * 32 + ((q ^ kb) << 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) stg[base + xe[e]] = acc[p][q][e];
      }
  }
  const bool wt = a.outFloats > 0 && a.outFloats < (1L << 29);   // 32-bit byte offsets
  float* outp = a.out + (size_t)part * a.outPartStride;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(outp, 0, wt ? (int)(a.outFloats * 4) : 0, 0x00020000);
  float4 v4[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lrow = u * 8 + (lane >> 3), q = lane & 7;
    v4[u] = *reinterpret_cast<const float4*>(&stg[lrow * 32 + ((q ^ (lrow & 7)) << 2)]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lrow = u * 8 + (lane >> 3), q = lane & 7;
    const float4 v = v4[u];
    const int row = row0 + wr * 32 + lrow;
    // stacked row -> (support, node): the forward's mixes take the stride of their A operand (N on the tight stack)
    const int stride = ROLE != 2 ? a.stackStride : a.Np;
    const int k = row / stride, n = row - k * stride;
    const bool ok = k < a.Ks && n < a.N;
    const size_t off = (size_t)colTile * a.sT + (size_t)n * a.sN + (size_t)k * a.sK + wc * 32 + q * 4;
    if (wt) {
      const u32x4 bits = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
      // a row outside the output: an offset beyond num_records - the store is dropped by the range check, no branch
      __builtin_amdgcn_raw_buffer_store_b128(bits, rsrc, ok ? (int)(off * 4) : (int)0x7ffffff0, 0, 16);   // aux 16 = sc1
    } else if (ok) {
      *reinterpret_cast<float4*>(outp + off) = v;
    }
  }
}

// -------------------------------------------------------------------------------------------------
// 5a''. the same mix with 64-row x 32-column tiles: small batches
// -------------------------------------------------------------------------------------------------
// The reference ships batch_size 16 (MultiATGCN.json:12).  There k_mix has 20 x 16 = 320 workgroups for 256 CUs - 64 CUs get
// two, the launch takes 20.6 us for a quarter of the B = 64 work (41 us).  With half-width column tiles there are 640
// workgroups (2.5 per CU, five waves per CU on average as before, but the longest CU holds 3 halves instead of 2 wholes).
// Same pipeline as k_mix (K-step 16 through LDS, two K-tiles ahead in registers, rotated rows); a wave owns 32 rows x 16
// columns = 2 x 1 accumulators, the B tile uses columns 0..31 of its 64-wide LDS rows (both halves of the workgroup request
// it - duplicate stores of equal values).  Launched for at most 16 column tiles (B <= 16: mix_half_tiles).
template <int ROLE>
__global__ __launch_bounds__(256) void k_mix_c32(MixArgs a) {
  __shared__ __attribute__((aligned(16))) float As[2][16 * 64];
  __shared__ __attribute__((aligned(16))) float Bs[2][16 * 64];
  int ct2, rowTile;     // column unit: half a column tile
  mix_tile_order(blockIdx.x, 2 * a.nColTiles, a.nRowTiles, rowTile, ct2);
  const int colTile = ct2 >> 1, half = ct2 & 1;
  const int row0 = rowTile * 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, j = lane & 15, kq = lane >> 4;
  const int kk = tid >> 4, sg = tid & 15, sgB = sg & 7;
  const int part = blockIdx.y;
  const float* ap = a.St + (size_t)part * a.aPartStride + (size_t)kk * a.ldS + row0 + sg * 4;
  const float* bp = a.X + (size_t)part * a.xPartStride + (size_t)colTile * a.xTileStride + (size_t)kk * a.ldX + half * 32 + sgB * 4;
  const int stPosA = kk * 64 + (((sg + 4 * (kk & 3)) & 15) << 2);
  const int stPosB = kk * 64 + (((sgB + 4 * (kk & 3)) & 15) << 2);
  const int last = a.nK - 1;
  auto ldA = [&](int t) { return *reinterpret_cast<const float4*>(ap + (size_t)min(t, last) * 16 * a.ldS); };
  auto ldB = [&](int t) { return *reinterpret_cast<const float4*>(bp + (size_t)min(t, last) * 16 * a.ldX); };
  float4 ra0, rb0, ra1, rb1;
  {
    const float4 a0 = ldA(0), b0 = ldB(0);
    __builtin_amdgcn_sched_barrier(0);
    ra0 = ldA(1); rb0 = ldB(1); ra1 = ldA(2); rb1 = ldB(2);
    __builtin_amdgcn_sched_barrier(0);
    *reinterpret_cast<float4*>(&As[0][stPosA]) = a0;
    *reinterpret_cast<float4*>(&Bs[0][stPosB]) = b0;
  }
  __syncthreads();
  f32x4 acc[2];
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1] = acc[0];
  const int rotA0 = (wr * 32 + j + 16 * kq) & 63, rotA1 = (wr * 32 + 16 + j + 16 * kq) & 63;
  const int rotB0 = (wc * 16 + j + 16 * kq) & 63;
  auto mma = [&](int cur) {
    const float* A = &As[cur][kq * 64];
    const float* Bm = &Bs[cur][kq * 64];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const float a0 = A[s4 * 256 + rotA0], a1 = A[s4 * 256 + rotA1];
      const float b0 = Bm[s4 * 256 + rotB0];
      acc[0] = MFMA16(a0, b0, acc[0]);
      acc[1] = MFMA16(a1, b0, acc[1]);
    }
  };
  for (int it = 0; it < a.nK; it += 2) {
    mma(0);
    *reinterpret_cast<float4*>(&As[1][stPosA]) = ra0;
    *reinterpret_cast<float4*>(&Bs[1][stPosB]) = rb0;
    ra0 = ldA(it + 3); rb0 = ldB(it + 3);
    __syncthreads();
    if (it + 1 < a.nK) {
      mma(1);
      *reinterpret_cast<float4*>(&As[0][stPosA]) = ra1;
      *reinterpret_cast<float4*>(&Bs[0][stPosB]) = rb1;
      ra1 = ldA(it + 4); rb1 = ldB(it + 4);
      __syncthreads();
    }
  }
  // epilogue: the wave's 32 x 16 tile through LDS ([32 rows][4 slots], slot ^ (row & 3)), 16-byte write-through stores
  float* stg = (w < 2 ? &As[0][0] : &Bs[0][0]) + (w & 1) * 1024;
  {
    const int jq = j >> 2, jr = j & 3;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int lrow = p * 16 + 4 * kq + e;
        stg[lrow * 16 + ((jq ^ (lrow & 3)) << 2) + jr] = acc[p][e];
      }
  }
  const bool wt = a.outFloats > 0 && a.outFloats < (1L << 29);
  float* outp = a.out + (size_t)part * a.outPartStride;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(outp, 0, wt ? (int)(a.outFloats * 4) : 0, 0x00020000);
  float4 v2[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int lrow = u * 16 + (lane >> 2), q = lane & 3;
    v2[u] = *reinterpret_cast<const float4*>(&stg[lrow * 16 + ((q ^ (lrow & 3)) << 2)]);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int lrow = u * 16 + (lane >> 2), q = lane & 3;
    const float4 v = v2[u];
    const int row = row0 + wr * 32 + lrow;
    const int k = row / a.Np, n = row - k * a.Np;
    const bool ok = k < a.Ks && n < a.N;
    const size_t off = (size_t)colTile * a.sT + (size_t)n * a.sN + (size_t)k * a.sK + half * 32 + wc * 16 + q * 4;
    if (wt) {
      const u32x4 bits = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
      __builtin_amdgcn_raw_buffer_store_b128(bits, rsrc, ok ? (int)(off * 4) : (int)0x7ffffff0, 0, 16);   // sc1; dropped when out of range
    } else if (ok) {
      *reinterpret_cast<float4*>(outp + off) = v;
    }
  }
}

// -------------------------------------------------------------------------------------------------
// 5a'. the same mix with a 32-row x 128-column workgroup tile (the backward's transposed mix)
// -------------------------------------------------------------------------------------------------
// The transposed mix has N = 403 output rows: 7 row tiles of 64 are 10 % padding and 7 x 64 x 3 parts = 1344 workgroups
// are 5.25 per CU (one CU in four runs a sixth round).  32-row tiles cover 416 rows (3 %), and with 128 columns - two
// batch rows - per workgroup 13 x 32 x 3 = 1248 workgroups are 4.9 per CU.  Each of the 4 waves owns 32 of the 128 columns
// and all 32 rows: the same 2 x 2 accumulators, K-tile 16, two tiles ahead in registers, rotated LDS rows (16 floats per odd
// k: the two k rows a 32-lane half reads sit half a bank row apart) and write-through row-store epilogue as k_mix.
// Needs an even number of column tiles (mix_backward_tile: k_mix<2> otherwise).
// BF (matgcn_set_train_precision(1|2), the training side line): bf16 OPERANDS, fp32 accumulation, on
// v_mfma_f32_16x16x32_bf16 - see k_mix_n32_bf_loop below; tiles, work split and epilogue are the fp32 kernel's.
__device__ __forceinline__ void k_mix_n32_bf_loop(const MixArgs& a, unsigned int (*As)[16 * 32], unsigned int (*Bs)[16 * 128],
                                                  int row0, int colPair, int part, f32x4 (&acc)[2][2]);
template <bool BF = false>
__global__ __launch_bounds__(256) void k_mix_n32(MixArgs a) {
  __shared__ __attribute__((aligned(16))) float As[2][16 * 32];
  __shared__ __attribute__((aligned(16))) float Bs[2][16 * 128];
  int colPair, rowTile;
  mix_tile_order(blockIdx.x, a.nColTiles >> 1, a.nRowTiles, rowTile, colPair);
  const int row0 = rowTile * 32;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int part = blockIdx.y;
  f32x4 acc[2][2];
  if constexpr (BF) {
    k_mix_n32_bf_loop(a, reinterpret_cast<unsigned int (*)[16 * 32]>(As), reinterpret_cast<unsigned int (*)[16 * 128]>(Bs),
                          row0, colPair, part, acc);
  } else {
  // staging: A tile 16 k x 32 rows = 128 float4 (threads t and t + 128 fetch and store the same one: no branch in the
  // pipeline), B tile 16 k x 128 columns = two float4 per thread (column tiles 2 colPair and 2 colPair + 1)
  const int akk = (tid & 127) >> 3, asg = tid & 7;
  const int bkk = tid >> 4, bsg = tid & 15;
  const float* ap = a.St + (size_t)part * a.aPartStride + (size_t)akk * a.ldS + row0 + asg * 4;
  const float* bp0 = a.X + (size_t)part * a.xPartStride + (size_t)(2 * colPair) * a.xTileStride + (size_t)bkk * a.ldX + bsg * 4;
  const float* bp1 = bp0 + a.xTileStride;
  const int aPos = akk * 32 + ((asg * 4 + 16 * (akk & 1)) & 31);
  const int bPos0 = bkk * 128 + ((bsg * 4 + 16 * (bkk & 1)) & 127);
  const int bPos1 = bkk * 128 + ((64 + bsg * 4 + 16 * (bkk & 1)) & 127);
  const int last = a.nK - 1;
  auto ldA = [&](int t) { return *reinterpret_cast<const float4*>(ap + (size_t)min(t, last) * 16 * a.ldS); };
  auto ldB0 = [&](int t) { return *reinterpret_cast<const float4*>(bp0 + (size_t)min(t, last) * 16 * a.ldX); };
  auto ldB1 = [&](int t) { return *reinterpret_cast<const float4*>(bp1 + (size_t)min(t, last) * 16 * a.ldX); };
  float4 ra0, rb00, rb01, ra1, rb10, rb11;   // (every request of the prologue before its first wait: see k_mix)
  {
    const float4 a0 = ldA(0), b0 = ldB0(0), b1 = ldB1(0);
    __builtin_amdgcn_sched_barrier(0);
    ra0 = ldA(1); rb00 = ldB0(1); rb01 = ldB1(1); ra1 = ldA(2); rb10 = ldB0(2); rb11 = ldB1(2);
    __builtin_amdgcn_sched_barrier(0);
    *reinterpret_cast<float4*>(&As[0][aPos]) = a0;
    *reinterpret_cast<float4*>(&Bs[0][bPos0]) = b0;
    *reinterpret_cast<float4*>(&Bs[0][bPos1]) = b1;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fragment of reduction index k = 4 s + kq: its row is rotated by 16 * (k & 1) = 16 * (kq & 1)
  const int rot = 16 * (kq & 1);
  const int cA0 = (j + rot) & 31, cA1 = (16 + j + rot) & 31;
  const int cB0 = (w * 32 + j + rot) & 127, cB1 = (w * 32 + 16 + j + rot) & 127;
  auto mma = [&](int cur) {
    const float* A = &As[cur][kq * 32];
    const float* Bm = &Bs[cur][kq * 128];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float a0 = A[s * 128 + cA0], a1 = A[s * 128 + cA1];
      const float b0 = Bm[s * 512 + cB0], b1 = Bm[s * 512 + cB1];
      acc[0][0] = MFMA16(a0, b0, acc[0][0]);
      acc[0][1] = MFMA16(a0, b1, acc[0][1]);
      acc[1][0] = MFMA16(a1, b0, acc[1][0]);
      acc[1][1] = MFMA16(a1, b1, acc[1][1]);
    }
  };
  for (int it = 0; it < a.nK; it += 2) {
    mma(0);                                               // tile it
    *reinterpret_cast<float4*>(&As[1][aPos]) = ra0;       // tile it+1 (a clamped copy past the end: unused)
    *reinterpret_cast<float4*>(&Bs[1][bPos0]) = rb00;
    *reinterpret_cast<float4*>(&Bs[1][bPos1]) = rb01;
    ra0 = ldA(it + 3); rb00 = ldB0(it + 3); rb01 = ldB1(it + 3);
    __syncthreads();
    if (it + 1 < a.nK) {
      mma(1);                                             // tile it+1
      *reinterpret_cast<float4*>(&As[0][aPos]) = ra1;     // tile it+2
      *reinterpret_cast<float4*>(&Bs[0][bPos0]) = rb10;
      *reinterpret_cast<float4*>(&Bs[0][bPos1]) = rb11;
      ra1 = ldA(it + 4); rb10 = ldB0(it + 4); rb11 = ldB1(it + 4);
      __syncthreads();
    }
  }
  }
  // epilogue as k_mix (batched, branch-free: round 4): the wave's 32 x 32 tile through LDS (Bs is free after the last
  // barrier), 16-byte write-through stores
  float* stg = &Bs[0][0] + w * 1024;
  {
    const int jq = j >> 2, jr = j & 3, kb = kq & 1;
    int xe[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) xe[e] = e * 32 + ((jq ^ e) << 2) + jr;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int base = (p * 16 + 4 * kq) * 32 + ((q ^ kb) << 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) stg[base + xe[e]] = acc[p][q][e];
      }
  }
  const bool wt = a.outFloats > 0 && a.outFloats < (1L << 29);   // 32-bit byte offsets
  float* outp = a.out + (size_t)part * a.outPartStride;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(outp, 0, wt ? (int)(a.outFloats * 4) : 0, 0x00020000);
  const int colTile = 2 * colPair + (w >> 1), wc = w & 1;
  float4 v4[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lrow = u * 8 + (lane >> 3), q = lane & 7;
    v4[u] = *reinterpret_cast<const float4*>(&stg[lrow * 32 + ((q ^ (lrow & 7)) << 2)]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lrow = u * 8 + (lane >> 3), q = lane & 7;
    const float4 v = v4[u];
    const int row = row0 + lrow;
    const int k = row / a.Np, n = row - k * a.Np;
    const bool ok = k < a.Ks && n < a.N;
    const size_t off = (size_t)colTile * a.sT + (size_t)n * a.sN + (size_t)k * a.sK + wc * 32 + q * 4;
    if (wt) {
      const u32x4 bits = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
      __builtin_amdgcn_raw_buffer_store_b128(bits, rsrc, ok ? (int)(off * 4) : (int)0x7ffffff0, 0, 16);   // sc1; dropped when out of range
    } else if (ok) {
      *reinterpret_cast<float4*>(outp + off) = v;
    }
  }
}

// -------------------------------------------------------------------------------------------------
// 5b. the same graph mix with bf16 OPERANDS (BASELINE config 3's dtype): fp32 accumulation, fp32 inputs and outputs
// -------------------------------------------------------------------------------------------------
// Opt-in variant (matgcn_set_mix_precision(1) / matgcn_set_train_precision(1): never the headline, narrower than the
// reference's fp32; ROLE 2: the backward's transposed mixes of odd row counts, split by slot like k_mix<2>).
// The supports and the state stay fp32 in memory; they are rounded to bf16 (round to nearest even) on their way into
// LDS, two consecutive reduction indices packed into one 32-bit word, so that a lane's v_mfma_f32_16x16x16_bf16
// fragment (4 consecutive k of one row / column) is two ds_read_b32.  K-tile 32 = 16 packed rows of 64 words; packed
// row p is rotated by 16 * ((p >> 1) & 3) words, which puts the four k-quarters of a wave on four different bank
// quarters.  Everything else - 64 x 64 tile, 2 x 2 accumulators per wave, register prefetch two tiles ahead, XCD-aware
// tile order, the write-through row-store epilogue - is k_mix's.
typedef short bf16x4_t __attribute__((ext_vector_type(4)));
#define MFMA16BF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ unsigned int bf16_rne(float x) {     // upper 16 bits of x, rounded to nearest even
  const unsigned int u = __float_as_uint(x);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint4 pack_bf16_rows(const float4& k0, const float4& k1) {   // word j = (k0[j], k1[j])
  return make_uint4(bf16_rne(k0.x) | (bf16_rne(k1.x) << 16), bf16_rne(k0.y) | (bf16_rne(k1.y) << 16),
                    bf16_rne(k0.z) | (bf16_rne(k1.z) << 16), bf16_rne(k0.w) | (bf16_rne(k1.w) << 16));
}
// The two fp32 rows behind packed row pr of K-tile t (32 reduction indices; nT tiles, kLast the last index): loads are
// unconditional (tile and row index clamped), values past the last reduction index zeroed by a select
__device__ __forceinline__ void mix_ld_bf16_pair(const float* base, size_t ld, int pr, int t, int nT, int kLast, float4& r0,
                                                 float4& r1) {
  const int k0 = 32 * min(t, nT - 1) + 2 * pr, k1 = k0 + 1;
  const float4 v0 = *reinterpret_cast<const float4*>(base + (size_t)min(k0, kLast) * ld);
  const float4 v1 = *reinterpret_cast<const float4*>(base + (size_t)min(k1, kLast) * ld);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  r0 = k0 <= kLast ? v0 : z;
  r1 = k1 <= kLast ? v1 : z;
}

// K loop of k_mix_n32<true>: K-tile 32 = 16 packed rows (word = bf16 of reduction indices 2 pr, 2 pr + 1, rounded to
// nearest even on the way into LDS; indices past the last one read as zero).  One v_mfma_f32_16x16x32_bf16 per
// accumulator and K-tile: lane (j, kq) reads the four words of packed rows 4 kq .. 4 kq + 3 in its row / column - the
// 8 consecutive k of its A and B fragments - and its accumulator holds rows 4 kq + e, column j, as the fp32 16x16x4 one.
// Rows pr with (pr >> 2) odd are rotated by 16 words (the two k groups a 32-lane half reads sit half a bank row apart).
// Register prefetch two K-tiles ahead, one barrier per tile, as the fp32 kernel.
typedef __bf16 bf16x8v_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void k_mix_n32_bf_loop(const MixArgs& a, unsigned int (*As)[16 * 32], unsigned int (*Bs)[16 * 128],
                                                  int row0, int colPair, int part, f32x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int apr = (tid & 127) >> 3, asg = tid & 7;   // A: packed row, 4-row segment (threads t, t + 128 duplicate)
  const int bpr = tid >> 4, bsg = tid & 15;          // B: packed row, 4-column segment in each of the two column tiles
  const int kLast = 16 * a.nK - 1;
  const int nT = (a.nK + 1) >> 1;
  const float* ap = a.St + (size_t)part * a.aPartStride + row0 + asg * 4;
  const float* bp0 = a.X + (size_t)part * a.xPartStride + (size_t)(2 * colPair) * a.xTileStride + bsg * 4;
  const float* bp1 = bp0 + a.xTileStride;
  const int aPos = apr * 32 + ((asg * 4 + 16 * ((apr >> 2) & 1)) & 31);
  const int bPos0 = bpr * 128 + ((bsg * 4 + 16 * ((bpr >> 2) & 1)) & 127);
  const int bPos1 = bpr * 128 + ((64 + bsg * 4 + 16 * ((bpr >> 2) & 1)) & 127);
  struct Tile { float4 a0, a1, b00, b01, b10, b11; };
  auto load = [&](int t, Tile& r) {
    mix_ld_bf16_pair(ap, a.ldS, apr, t, nT, kLast, r.a0, r.a1);
    mix_ld_bf16_pair(bp0, a.ldX, bpr, t, nT, kLast, r.b00, r.b01);
    mix_ld_bf16_pair(bp1, a.ldX, bpr, t, nT, kLast, r.b10, r.b11);
  };
  auto store = [&](int buf, const Tile& r) {
    *reinterpret_cast<uint4*>(&As[buf][aPos]) = pack_bf16_rows(r.a0, r.a1);
    *reinterpret_cast<uint4*>(&Bs[buf][bPos0]) = pack_bf16_rows(r.b00, r.b01);
    *reinterpret_cast<uint4*>(&Bs[buf][bPos1]) = pack_bf16_rows(r.b10, r.b11);
  };
  Tile r0, r1, r2;
  load(0, r0);
  load(1, r1);
  load(2, r2);
  store(0, r0);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int rot = 16 * (kq & 1);
  const int cA0 = (j + rot) & 31, cA1 = (16 + j + rot) & 31;
  const int cB0 = (w * 32 + j + rot) & 127, cB1 = (w * 32 + 16 + j + rot) & 127;
  auto frag = [&](const unsigned int* T, int width, int c) {
    const uint4 u = make_uint4(T[(4 * kq) * width + c], T[(4 * kq + 1) * width + c], T[(4 * kq + 2) * width + c],
                               T[(4 * kq + 3) * width + c]);
    return __builtin_bit_cast(bf16x8v_t, u);
  };
  auto mma = [&](int cur) {
    const bf16x8v_t fa0 = frag(As[cur], 32, cA0), fa1 = frag(As[cur], 32, cA1);
    const bf16x8v_t fb0 = frag(Bs[cur], 128, cB0), fb1 = frag(Bs[cur], 128, cB1);
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0, fb0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0, fb1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1, fb0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1, fb1, acc[1][1], 0, 0, 0);
  };
  for (int it = 0; it < nT; it += 2) {
    mma(0);                 // tile it
    store(1, r1);           // tile it+1 (a clamped copy past the end: unused)
    load(it + 3, r1);
    __syncthreads();
    if (it + 1 < nT) {
      mma(1);               // tile it+1
      store(0, r2);         // tile it+2
      load(it + 4, r2);
      __syncthreads();
    }
  }
}

// k_mix's store epilogue (see there for its measured reasons) as a function: the wave's 32 x 32 accumulator tile - rows
// row0 .., columns col0 .. of column tile colTile - through its 4 KB of LDS at stg into write-through row stores.  The fp32
// kernels keep theirs inline: behind a call the compiler requests the epilogue's kernel arguments in front of the K loop,
// 9 more scalar registers and another schedule for kernels whose code is pinned (variant tables).
__device__ __forceinline__ void mix_store_tile(const MixArgs& a, int part, float* stg, const f32x4 (&acc)[2][2], int row0,
                                               int colTile, int col0) {
  const int lane = threadIdx.x & 63, j = lane & 15, kq = lane >> 4;
  const int jq = j >> 2, jr = j & 3, kb = kq & 1;
  int xe[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) xe[e] = e * 32 + ((jq ^ e) << 2) + jr;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int base = (p * 16 + 4 * kq) * 32 + ((q ^ kb) << 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) stg[base + xe[e]] = acc[p][q][e];
    }
  const bool wt = a.outFloats > 0 && a.outFloats < (1L << 29);   // 32-bit byte offsets
  float* outp = a.out + (size_t)part * a.outPartStride;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(outp, 0, wt ? (int)(a.outFloats * 4) : 0, 0x00020000);
  float4 v4[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lrow = u * 8 + (lane >> 3), q = lane & 7;
    v4[u] = *reinterpret_cast<const float4*>(&stg[lrow * 32 + ((q ^ (lrow & 7)) << 2)]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lrow = u * 8 + (lane >> 3), q = lane & 7;
    const float4 v = v4[u];
    const int row = row0 + lrow;
    const int k = row / a.Np, n = row - k * a.Np;
    const bool ok = k < a.Ks && n < a.N;
    const size_t off = (size_t)colTile * a.sT + (size_t)n * a.sN + (size_t)k * a.sK + col0 + q * 4;
    if (wt) {
      const u32x4 bits = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
      __builtin_amdgcn_raw_buffer_store_b128(bits, rsrc, ok ? (int)(off * 4) : (int)0x7ffffff0, 0, 16);   // sc1; dropped when out of range
    } else if (ok) {
      *reinterpret_cast<float4*>(outp + off) = v;
    }
  }
}

template <int ROLE>
__global__ __launch_bounds__(256) void k_mix_bf16(MixArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned int As[2][16 * 64];
  __shared__ __attribute__((aligned(16))) unsigned int Bs[2][16 * 64];
  int colTile, rowTile;
  mix_tile_order(blockIdx.x, a.nColTiles, a.nRowTiles, rowTile, colTile);
  const int row0 = rowTile * 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, j = lane & 15, kq = lane >> 4;
  const int pr = tid >> 4, sg = tid & 15;                  // staging: packed row pr (k = 2 pr, 2 pr + 1), 4-word segment sg
  const int kLast = 16 * a.nK - 1;                         // reduction indices 0 .. Np-1 (a.nK = Np / 16)
  const int nT = (a.nK + 1) >> 1;                          // K-tiles of 32
  const int stPos = pr * 64 + (((sg + 4 * ((pr >> 1) & 3)) & 15) << 2);
  // split reduction (ROLE 2, the backward's transposed mix, MixArgs.parts): part p reads its own rows, writes its own output
  const int part = ROLE == 2 ? (int)blockIdx.y : 0;
  const float* ap = a.St + (size_t)part * a.aPartStride + row0 + sg * 4;
  const float* bp = a.X + (size_t)part * a.xPartStride + (size_t)colTile * a.xTileStride + sg * 4;
  auto ld = [&](const float* base, size_t ld_, int t, float4& r0, float4& r1) { mix_ld_bf16_pair(base, ld_, pr, t, nT, kLast, r0, r1); };
  float4 a0, a1, b0, b1, a2, a3, b2, b3;
  ld(ap, a.ldS, 0, a0, a1); ld(bp, a.ldX, 0, b0, b1);
  *reinterpret_cast<uint4*>(&As[0][stPos]) = pack_bf16_rows(a0, a1);
  *reinterpret_cast<uint4*>(&Bs[0][stPos]) = pack_bf16_rows(b0, b1);
  ld(ap, a.ldS, 1, a0, a1); ld(bp, a.ldX, 1, b0, b1);      // tile t+1 waits in (a0, a1, b0, b1) / (a2, a3, b2, b3)
  ld(ap, a.ldS, 2, a2, a3); ld(bp, a.ldX, 2, b2, b3);
  __syncthreads();
  f32x4 acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  // word of packed row (8 s + 2 kq + h) for row / column x: rotation 16 * kq
  const int rotA0 = (wr * 32 + j + 16 * kq) & 63, rotA1 = (wr * 32 + 16 + j + 16 * kq) & 63;
  const int rotB0 = (wc * 32 + j + 16 * kq) & 63, rotB1 = (wc * 32 + 16 + j + 16 * kq) & 63;
  auto frag = [&](const unsigned int* T, int s, int rot) {
    const unsigned int lo = T[(8 * s + 2 * kq) * 64 + rot], hi = T[(8 * s + 2 * kq + 1) * 64 + rot];
    bf16x4_t v;
    v[0] = (short)(lo & 0xffffu); v[1] = (short)(lo >> 16); v[2] = (short)(hi & 0xffffu); v[3] = (short)(hi >> 16);
    return v;
  };
  auto mma = [&](int cur) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {      // the two 16-wide k-steps of this K-tile
      const bf16x4_t fa0 = frag(As[cur], s, rotA0), fa1 = frag(As[cur], s, rotA1);
      const bf16x4_t fb0 = frag(Bs[cur], s, rotB0), fb1 = frag(Bs[cur], s, rotB1);
      acc[0][0] = MFMA16BF(fa0, fb0, acc[0][0]);
      acc[0][1] = MFMA16BF(fa0, fb1, acc[0][1]);
      acc[1][0] = MFMA16BF(fa1, fb0, acc[1][0]);
      acc[1][1] = MFMA16BF(fa1, fb1, acc[1][1]);
    }
  };
  for (int it = 0; it < nT; it += 2) {
    mma(0);
    *reinterpret_cast<uint4*>(&As[1][stPos]) = pack_bf16_rows(a0, a1);
    *reinterpret_cast<uint4*>(&Bs[1][stPos]) = pack_bf16_rows(b0, b1);
    ld(ap, a.ldS, it + 3, a0, a1); ld(bp, a.ldX, it + 3, b0, b1);
    __syncthreads();
    if (it + 1 < nT) {
      mma(1);
      *reinterpret_cast<uint4*>(&As[0][stPos]) = pack_bf16_rows(a2, a3);
      *reinterpret_cast<uint4*>(&Bs[0][stPos]) = pack_bf16_rows(b2, b3);
      ld(ap, a.ldS, it + 4, a2, a3); ld(bp, a.ldX, it + 4, b2, b3);
      __syncthreads();
    }
  }
  mix_store_tile(a, part, reinterpret_cast<float*>(w < 2 ? &As[0][0] : &Bs[0][0]) + (w & 1) * 1024, acc, row0 + wr * 32,
                 colTile, wc * 32);
}

// -------------------------------------------------------------------------------------------------
// 5c. the same graph mix as THREE bf16 pieces per operand (matgcn_set_mix_precision(3)): fp32 accuracy on the bf16 pipe
// -------------------------------------------------------------------------------------------------
// x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (both differences are exact in fp32;
// the three pieces carry 24 significand bits).  S.X is the sum of nine piece products; the six leading ones - hi.lo,
// lo.hi, mid.mid, hi.mid, mid.hi, hi.hi, issued in that order: smallest first - are accumulated in fp32 on
// v_mfma_f32_16x16x32_bf16, the three dropped ones (mid.lo, lo.mid, lo.lo) are at most about 2^-24 relative each.
// Workgroup tile 64 rows x 128 columns (a PAIR of column tiles, as k_mix_n32: half the St bytes per output of the 64-wide
// kernels), 4 waves of 32 rows x 64 columns = 2 x 4 accumulators; K-tile 32 = 4 k-groups of 8 consecutive reduction indices,
// one 16-byte word per (piece, k-group, row or column), which is exactly a lane's MFMA fragment: one ds_read_b128,
// conflict-free (the 16 lanes of a read group take 16 consecutive words of one 256-byte bank row or two disjoint runs of them).
//   A: St is split ONCE per forward by k_split_bf16x3 into three planes of such words in the workspace; staging is a copy.
//   B: the state rows stay fp32 in memory (the node kernels and their bits are untouched); a thread fetches 8 k x 2 columns
//      of the next K-tile into registers while the current one is multiplied and splits them on their way into LDS
//      (v_cvt_pk_bf16_f32: 11 vector instructions per two values).
// LDS 36 KB per workgroup, ONE buffer (two barriers per K-tile); the next tile waits in registers.  Registers, not LDS,
// set the occupancy: 136 of 512 (164 with FLUSH) let three workgroups share a CU and cover each other's barriers, and a
// second buffer (3 x 72 KB > 160 KB) would cost the third.  An odd number of column tiles: the last pair's second half is fetched
// from the first (clamped) and not stored.  FLUSH as k_mix: partial sums every 8 K-tiles (256 reduction indices), N > 1024.
// Tile order and the store epilogue are the shared ones (mix_tile_order, mix_store_tile: twice per wave, 32 columns each).
// ROLE 2 (matgcn_set_train_bf16x3: the backward's transposed mixes on the plain stack StP [Ks*Np][NpC], launch_mix_plain):
// the reduction runs over support slots of Np indices each, and Np is a multiple of 16, not of the K-tile's 32 - the last
// K-tile of a slot must not run into the next slot's first 16 rows, which are not zero.  ONE plane layout for every
// role-2 launch: planes[piece][slot][nKg][NpC] words, every slot's Np reduction indices rounded up to 32 and zero-filled
// (k_split_bf16x3 per slot, nKg = 4 K-tiles-per-slot), so slot k's K-tile t is K-tile k * nT + t of the planes; the B rows
// of a slot's last K-tile are clamped to the slot's last row, where the planes hold zeros.  a.nK counts ONE slot's groups
// of 16; a workgroup walks a.kSlots slots back to back: 1 when the launch splits the reduction by slot (part =
// blockIdx.y: planes a.aPartStride WORDS, B rows a.xPartStride and output a.outPartStride floats further per part),
// all Ks of them when it does not (parts == 1).  FLUSH counts K-tiles across the slots of a part.
typedef __bf16 bf16x2v_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned int pack_bf16_pair(float lo, float hi) {    // round to nearest even, lo in bits 0..15
  const bf16x2v_t v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned int, v);
}
// pieces of (x0, x1) as three packed words
__device__ __forceinline__ void split_bf16x3(float x0, float x1, unsigned int& h, unsigned int& m, unsigned int& l) {
  h = pack_bf16_pair(x0, x1);
  x0 -= __uint_as_float(h << 16); x1 -= __uint_as_float(h & 0xffff0000u);
  m = pack_bf16_pair(x0, x1);
  x0 -= __uint_as_float(m << 16); x1 -= __uint_as_float(m & 0xffff0000u);
  l = pack_bf16_pair(x0, x1);
}

// St [Np][ldS] -> planes[piece][Np32 / 8][ldS] words; reduction indices >= Np read as zero
__global__ __launch_bounds__(256) void k_split_bf16x3(const float* __restrict__ St, int ldS, int Np, int nKg,
                                                      uint4* __restrict__ planes, long plStride) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)nKg * ldS) return;
  const int kg = (int)(id / ldS), col = (int)(id - (size_t)kg * ldS);
  unsigned int h[4], m[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k0 = 8 * kg + 2 * i, k1 = k0 + 1;
    const float x0 = k0 < Np ? St[(size_t)k0 * ldS + col] : 0.f;
    const float x1 = k1 < Np ? St[(size_t)k1 * ldS + col] : 0.f;
    split_bf16x3(x0, x1, h[i], m[i], l[i]);
  }
  planes[id] = make_uint4(h[0], h[1], h[2], h[3]);
  planes[plStride + id] = make_uint4(m[0], m[1], m[2], m[3]);
  planes[2 * plStride + id] = make_uint4(l[0], l[1], l[2], l[3]);
}

template <int ROLE, bool FLUSH = false>
__global__ __launch_bounds__(256) void k_mix_bf16x3(MixArgs a) {
  __shared__ __attribute__((aligned(16))) u32x4 As[3][4][64];     // [piece][k-group][row]
  __shared__ __attribute__((aligned(16))) u32x4 Bs[3][4][128];    // [piece][k-group][column]
  int colPair, rowTile;
  mix_tile_order(blockIdx.x, (a.nColTiles + 1) >> 1, a.nRowTiles, rowTile, colPair);
  const int row0 = rowTile * 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1, j = lane & 15, kq = lane >> 4;
  const int kLast = 16 * a.nK - 1;                         // reduction indices 0 .. Np-1 (a.nK = Np / 16)
  const int nT = (a.nK + 1) >> 1;                          // K-tiles of 32 (ROLE 2: of one slot)
  const int nTot = ROLE == 2 ? a.kSlots * nT : nT;         // K-tiles of this workgroup's reduction
  const int part = ROLE == 2 ? (int)blockIdx.y : 0;
  // staging: k-group skg of the tile; A row sr (one word per piece), B columns 2 sr, 2 sr + 1 of the 128
  const int skg = tid >> 6, sr = tid & 63;
  const u32x4* ap = reinterpret_cast<const u32x4*>(a.Apl) + (size_t)skg * a.ldS + row0 + sr;
  const int bcol = 2 * sr;
  const int bTile = min(2 * colPair + (bcol >> 6), a.nColTiles - 1);
  const float* bp = a.X + (size_t)bTile * a.xTileStride + (bcol & 63);
  if constexpr (ROLE == 2) {
    ap += (size_t)part * a.aPartStride;
    bp += (size_t)part * a.xPartStride;
  }
  u32x4 ra[3];
  float2 rb[8];
  int nxSlot = 0, nxT = 0;       // ROLE 2: slot, and K-tile within it, of the next load (the loads come in tile order)
  auto load = [&](int t) {
    if constexpr (ROLE == 2) {
      const int tc = nxSlot * nT + nxT, rowBase = nxSlot * 16 * a.nK;
#pragma unroll
      for (int p = 0; p < 3; ++p) ra[p] = ap[(size_t)p * a.plStride + (size_t)tc * 4 * a.ldS];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        // (past the slot's last index: its last row again - the planes are zero there, the next slot's rows are not)
        rb[i] = *reinterpret_cast<const float2*>(bp + (size_t)(rowBase + min(32 * nxT + 8 * skg + i, kLast)) * a.ldX);
      }
      if (t + 1 < nTot && ++nxT == nT) { nxT = 0; ++nxSlot; }   // (clamped past the end: the last tile again, unused)
    } else {
      const int tc = min(t, nT - 1);
#pragma unroll
      for (int p = 0; p < 3; ++p) ra[p] = ap[(size_t)p * a.plStride + (size_t)tc * 4 * a.ldS];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        // (a reduction index past the last one repeats the last row: its St words are zero in every plane)
        rb[i] = *reinterpret_cast<const float2*>(bp + (size_t)min(32 * tc + 8 * skg + i, kLast) * a.ldX);
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int p = 0; p < 3; ++p) As[p][skg][sr] = ra[p];
    unsigned int h0[4], m0[4], l0[4], h1[4], m1[4], l1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      split_bf16x3(rb[2 * i].x, rb[2 * i + 1].x, h0[i], m0[i], l0[i]);
      split_bf16x3(rb[2 * i].y, rb[2 * i + 1].y, h1[i], m1[i], l1[i]);
    }
    Bs[0][skg][bcol] = u32x4{h0[0], h0[1], h0[2], h0[3]};
    Bs[0][skg][bcol + 1] = u32x4{h1[0], h1[1], h1[2], h1[3]};
    Bs[1][skg][bcol] = u32x4{m0[0], m0[1], m0[2], m0[3]};
    Bs[1][skg][bcol + 1] = u32x4{m1[0], m1[1], m1[2], m1[3]};
    Bs[2][skg][bcol] = u32x4{l0[0], l0[1], l0[2], l0[3]};
    Bs[2][skg][bcol + 1] = u32x4{l1[0], l1[1], l1[2], l1[3]};
  };
  load(0);
  store();
  load(1);
  __syncthreads();
  f32x4 acc[2][2][2], tot[FLUSH ? 2 : 1][4];   // acc[q >> 1][p][q & 1]: a half is one call of the store epilogue
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc[q >> 1][p][q & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (FLUSH) tot[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  auto fragA = [&](int piece, int p) { return __builtin_bit_cast(bf16x8v_t, As[piece][kq][wr * 32 + p * 16 + j]); };
  auto fragB = [&](int piece, int q) { return __builtin_bit_cast(bf16x8v_t, Bs[piece][kq][wc * 64 + q * 16 + j]); };
  auto mma = [&]() {
    bf16x8v_t fa[3][2];
#pragma unroll
    for (int piece = 0; piece < 3; ++piece)
#pragma unroll
      for (int p = 0; p < 2; ++p) fa[piece][p] = fragA(piece, p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bf16x8v_t bh = fragB(0, q), bm = fragB(1, q), bl = fragB(2, q);
      // smallest terms first; the two row blocks alternate so that consecutive MFMAs are independent
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[q >> 1][p][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][p], bl, acc[q >> 1][p][q & 1], 0, 0, 0);
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[q >> 1][p][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[2][p], bh, acc[q >> 1][p][q & 1], 0, 0, 0);
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[q >> 1][p][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1][p], bm, acc[q >> 1][p][q & 1], 0, 0, 0);
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[q >> 1][p][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][p], bm, acc[q >> 1][p][q & 1], 0, 0, 0);
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[q >> 1][p][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1][p], bh, acc[q >> 1][p][q & 1], 0, 0, 0);
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[q >> 1][p][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][p], bh, acc[q >> 1][p][q & 1], 0, 0, 0);
    }
  };
  for (int t = 0; t < nTot; ++t) {
    mma();                       // tile t
    __syncthreads();             // every wave has read tile t
    if (t + 1 < nTot) {
      store();                   // tile t+1
      load(t + 2);               // (clamped past the end: unused)
    }
    __syncthreads();
    if constexpr (FLUSH) {
      if (((t + 1) & (MIX_FLUSH_TILES / 2 - 1)) == 0) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) tot[p][q][e] += acc[q >> 1][p][q & 1][e];
            acc[q >> 1][p][q & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
  }
  if constexpr (FLUSH) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q >> 1][p][q & 1][e] += tot[p][q][e];
  }
  // the wave's 32 x 64 tile lies in ONE column tile: two passes of the shared epilogue through the wave's 4 KB of Bs
  // (free after the loop's last barrier)
  const int colTile = 2 * colPair + wc;
  if (colTile < a.nColTiles) {
    float* stg = reinterpret_cast<float*>(&Bs[0][0][0]) + w * 1024;
#pragma unroll
    for (int half = 0; half < 2; ++half) mix_store_tile(a, part, stg, acc[half], row0 + wr * 32, colTile, half * 32);
  }
}

// =================================================================================================
// 8. output head (MultiATGCN.py:416-418): Conv2d(T -> out*od, (1,H)) == [B*N x T*H] . [T*H x CH]
// =================================================================================================
// One workgroup of 4 waves per (b, 32-node tile): the waves split the T steps of the reduction (t = w, w+4, ..)
// so four times as many loads are in flight per tile, and add their partial tiles in LDS in a fixed order.
// A fragments come straight from the padded time-major sequence [T][B][Np][64] (each lane walks its node's
// 256-byte rows), B = fragment-ordered conv weight from L2.  out[b][o][n][dd] with channel ch = o*od + dd.
__global__ __launch_bounds__(256) void k_head(HeadArgs a) {
  __shared__ f32x16 part[3][2][64];      // partial accumulators of waves 1..3
  const int tilesPerB = (a.N + 31) >> 5;
  const int b = blockIdx.x / tilesPerB, n0 = (blockIdx.x % tilesPerB) * 32;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  const int node = min(n0 + i, a.Np - 1);  // pad rows are zero / in bounds
  f32x16 acc[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tt][r] = 0.f;
  const int nt = a.NTc;
  for (int t = w; t < a.T; t += 4) {
    const float* rowp = a.seq + (((size_t)t * a.B + b) * a.Np + node) * 64 + half * 4;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const float4 a4 = *reinterpret_cast<const float4*>(rowp + g * 8);
      const int jg = t * 8 + g;
      for (int tt = 0; tt < nt; ++tt) {
        const float4 w4 = *reinterpret_cast<const float4*>(a.w + ((size_t)(jg * nt + tt) * 64 + lane) * 4);
        acc[tt] = MFMA32(a4.x, w4.x, acc[tt]);
        acc[tt] = MFMA32(a4.y, w4.y, acc[tt]);
        acc[tt] = MFMA32(a4.z, w4.z, acc[tt]);
        acc[tt] = MFMA32(a4.w, w4.w, acc[tt]);
      }
    }
  }
  if (w > 0) { part[w - 1][0][lane] = acc[0]; part[w - 1][1][lane] = acc[1]; }
  __syncthreads();
  if (w > 0) return;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const f32x16 p0 = part[q][0][lane], p1 = part[q][1][lane];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] += p0[r]; acc[1][r] += p1[r]; }
  }
  // accumulator rows = nodes, cols = channels
  for (int tt = 0; tt < nt; ++tt) {
    const int ch = tt * 32 + i;
    if (ch >= a.CH) continue;
    const float bias = a.bias[ch];
    const int o = ch / a.od, dd = ch - o * a.od;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + acc_row(r, half);
      if (n < a.N) a.out[(((size_t)b * (a.CH / a.od) + o) * a.N + n) * a.od + dd] = acc[tt][r] + bias;
    }
  }
}

// ---- the head over S dropout masks (matgcn_forward_mc: Monte-Carlo dropout) ---------------------------------------------
// k_head's product repeated over the samples: the same grid, the same split of the T steps over the four waves, the same
// MFMA order per accumulator and the same fixed order of the partial sums in LDS - sample s is, bit for bit, what k_head
// gives on seq * mask_s.  The mask never exists: a lane's float4 of A is multiplied by the four multipliers of one Philox
// call (matgcn_philox.h) as it enters the MFMAs.
// Register / LDS choice: a workgroup's A tile is T * 32 * 64 * 4 = 196 608 bytes - more than the 160 KB of LDS - but per
// LANE it is 6 steps x 8 float4 = 192 values, and the kernel runs one wave per SIMD (__launch_bounds__(256): a budget of
// 512 registers), so the tile is loaded ONCE into VGPRs and every sample re-reads only the conv weight (L2-resident,
// 96 KB per wave).  Wave 0 keeps the running mean and M2 of its 32 outputs per lane (Welford, fp32; the count is the
// sample index) in 16 KB of lane-private LDS - with them in registers as well the kernel spilled 784 bytes per lane to
// scratch - and writes mean and the population standard deviation when the samples are done.
constexpr int HEAD_MC_STEPS = 6;   // steps per wave held in registers: headT <= 24 (checked by the launcher)
template <int K> struct HeadStep { static constexpr int value = K; };
__global__ __launch_bounds__(256) void k_head_mc(HeadMcArgs m) {
  const HeadArgs& a = m.h;
  __shared__ f32x16 part[3][2][64];      // partial accumulators of waves 1..3
  __shared__ float stat[2][32][64];      // wave 0: running mean [0] and M2 [1] of its 32 outputs per lane (lane-private)
  const int tilesPerB = (a.N + 31) >> 5;
  const int b = blockIdx.x / tilesPerB, n0 = (blockIdx.x % tilesPerB) * 32;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = lane & 31, half = lane >> 5;
  const int node = min(n0 + i, a.Np - 1);  // pad rows are zero / in bounds
  const int nt = a.NTc;
  float4 av[HEAD_MC_STEPS][8];
#pragma unroll
  for (int k = 0; k < HEAD_MC_STEPS; ++k) {
    const int t = w + 4 * k;
    const float* rowp = a.seq + (((size_t)min(t, a.T - 1) * a.B + b) * a.Np + node) * 64 + half * 4;
#pragma unroll
    for (int g = 0; g < 8; ++g) av[k][g] = *reinterpret_cast<const float4*>(rowp + g * 8);
  }
  float bias[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) bias[tt] = (tt < nt && tt * 32 + i < a.CH) ? a.bias[tt * 32 + i] : 0.f;
  if (w == 0) {
#pragma unroll
    for (int e = 0; e < 32; ++e) { stat[0][e][lane] = 0.f; stat[1][e][lane] = 0.f; }
  }
  const size_t sampleFloats = (size_t)a.B * a.CH * a.N;
  // The conv weight is the same for every sample, and a loop-invariant load is hoisted: all 96 float4 of a wave ended up
  // live across the sample loop (512 registers, 928 bytes of scratch per lane in the ISA).  So the weight's base is made
  // opaque once per sample, the fragments of group g + 1 are requested while group g multiplies (8 MFMAs of 16 passes and
  // one Philox call cover an L2 hit), and a scheduling barrier per group keeps the requests from piling up.
  const int tFirst = min(w, a.T - 1);
  auto wload = [&](const float* wbase, int jg, float4 (&dst)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
      dst[tt] = *reinterpret_cast<const float4*>(wbase + ((size_t)(jg * nt + min(tt, nt - 1)) * 64 + lane) * 4);
  };
  float4 wc[2];
  wload(a.w, tFirst * 8, wc);
  const unsigned long long qLane = ((unsigned long long)b * a.T * a.N + (n0 + i)) * 16 + half;   // mask quad of step 0, g = 0
  for (int s = 0; s < m.samples; ++s) {
    DropDesc d = m.drop;
    d.offset += (unsigned long long)s;
    const float* wbase = a.w;
    asm volatile("" : "+s"(wbase));
    // (likewise the lane's mask position: the counters of all 48 calls and their first-round products are the same for
    // every sample and were kept live across the loop - about 200 registers)
    unsigned int qlo = (unsigned int)qLane, qhi = (unsigned int)(qLane >> 32);
    asm volatile("" : "+v"(qlo), "+v"(qhi));
    const unsigned long long qb = ((unsigned long long)qhi << 32) | qlo;
    f32x16 acc[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tt][r] = 0.f;
    // (one call per step with the step as a compile-time constant: left to `#pragma unroll` the compiler kept part of the
    // loop rolled, which made av[k] a runtime index and moved the whole tile to scratch)
    auto step = [&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      const int t = w + 4 * k;
      if (t < a.T) {   // wave-uniform
        // mask quad of (b, t, n0 + i, 8 g + 4 half .. + 3): position arithmetic only, rows past N decide nothing written
        const unsigned long long q0 = qb + (unsigned long long)t * a.N * 16;
        const int tNext = t + 4 < a.T ? t + 4 : tFirst;   // behind the wave's last step: the next sample's first group
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          float4 wn[2];
          wload(wbase, (g < 7 ? t : tNext) * 8 + ((g + 1) & 7), wn);
          const float4 mk = drop_mult4(d, q0 + 2 * g);
          const float4 a4 = make_float4(av[k][g].x * mk.x, av[k][g].y * mk.y, av[k][g].z * mk.z, av[k][g].w * mk.w);
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            if (tt < nt) {
              acc[tt] = MFMA32(a4.x, wc[tt].x, acc[tt]);
              acc[tt] = MFMA32(a4.y, wc[tt].y, acc[tt]);
              acc[tt] = MFMA32(a4.z, wc[tt].z, acc[tt]);
              acc[tt] = MFMA32(a4.w, wc[tt].w, acc[tt]);
            }
          }
          wc[0] = wn[0]; wc[1] = wn[1];
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    };
    static_assert(HEAD_MC_STEPS == 6, "one call per step below");
    step(HeadStep<0>{}); step(HeadStep<1>{}); step(HeadStep<2>{}); step(HeadStep<3>{}); step(HeadStep<4>{});
    step(HeadStep<5>{});
    if (w > 0) { part[w - 1][0][lane] = acc[0]; part[w - 1][1][lane] = acc[1]; }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const f32x16 p0 = part[q][0][lane], p1 = part[q][1][lane];
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] += p0[r]; acc[1][r] += p1[r]; }
      }
      const float inv = 1.0f / (float)(s + 1);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int ch = tt * 32 + i;
        const int o = ch / a.od, dd = ch - o * a.od;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float x = acc[tt][r] + bias[tt];
          const float mu0 = stat[0][tt * 16 + r][lane];
          const float delta = x - mu0;
          const float mu1 = mu0 + delta * inv;
          stat[0][tt * 16 + r][lane] = mu1;
          stat[1][tt * 16 + r][lane] += delta * (x - mu1);
          const int n = n0 + acc_row(r, half);
          if (m.samplesOut && tt < nt && ch < a.CH && n < a.N)
            m.samplesOut[s * sampleFloats + (((size_t)b * (a.CH / a.od) + o) * a.N + n) * a.od + dd] = x;
        }
      }
    }
    __syncthreads();   // the partial tiles are free for the next sample
  }
  if (w > 0) return;
  const float invS = 1.0f / (float)m.samples;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int ch = tt * 32 + i;
    if (tt >= nt || ch >= a.CH) continue;
    const int o = ch / a.od, dd = ch - o * a.od;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + acc_row(r, half);
      if (n >= a.N) continue;
      const size_t at = (((size_t)b * (a.CH / a.od) + o) * a.N + n) * a.od + dd;
      m.mean[at] = stat[0][tt * 16 + r][lane];
      m.stdev[at] = sqrtf(stat[1][tt * 16 + r][lane] * invS);
    }
  }
}

// =================================================================================================
// 9. loss / metric epilogue (MultiATGCN.py:422-427, loss.py:17-29, traffic_state_evaluator.py:87-104)
// =================================================================================================
// stage 1: one workgroup per (b, horizon): sum |p-l|*mask and sum mask over the N*od values of that slab
// (labelStart != null: y is the raw series (steps, N, yFeat), label row (b, o) = y[labelStart[b] + o])
__global__ __launch_bounds__(256) void k_mae_partial(const float* __restrict__ pred, const float* __restrict__ y,
                                                     const int* __restrict__ labelStart, int outSteps, int N, int od,
                                                     int ySteps, int yFeat, int yStart, float mean, float std,
                                                     float nullVal, float minS, float* __restrict__ partials) {
  __shared__ float sAbs[256], sCnt[256];
  const int b = blockIdx.x / outSteps, o = blockIdx.x - b * outSteps;
  const float* pp = pred + ((size_t)b * outSteps + o) * N * od;
  const size_t yrow = labelStart ? series_row((long)labelStart[b] + o, ySteps) : (size_t)b * ySteps + o;
  const float* yp = y + yrow * N * yFeat + yStart;
  const bool nanMask = nullVal != nullVal;
  float sa = 0.f, sc = 0.f;
  for (int idx = threadIdx.x; idx < N * od; idx += 256) {
    const int n = idx / od, c = idx - n * od;
    float l = yp[(size_t)n * yFeat + c] * std + mean;
    const float p = pp[idx] * std + mean;
    if (fabsf(l) < minS) l = 0.f;                       // loss.py:18 (the reference does this in place)
    const float m = nanMask ? (l == l ? 1.f : 0.f) : (l != nullVal ? 1.f : 0.f);
    const float d = fabsf(p - l) * m;
    sa += (d == d) ? d : 0.f;                           // nan -> 0 (loss.py:27)
    sc += m;
  }
  sAbs[threadIdx.x] = sa; sCnt[threadIdx.x] = sc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { sAbs[threadIdx.x] += sAbs[threadIdx.x + s]; sCnt[threadIdx.x] += sCnt[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = sAbs[0]; partials[2 * blockIdx.x + 1] = sCnt[0]; }
}

// stage 2: one workgroup: thread o sums horizon o over the batch in fp64, thread 0 then the total
__global__ __launch_bounds__(64) void k_mae_final(const float* __restrict__ partials, int B, int outSteps,
                                                  float* __restrict__ result) {
  __shared__ double hAbs[64], hCnt[64];
  const int o = threadIdx.x;
  double sa = 0.0, sc = 0.0;
  if (o < outSteps)
    for (int b = 0; b < B; ++b) { sa += partials[2 * (b * outSteps + o)]; sc += partials[2 * (b * outSteps + o) + 1]; }
  hAbs[o] = sa; hCnt[o] = sc;
  if (o < outSteps) result[1 + o] = sc > 0.0 ? (float)(sa / sc) : 0.f;
  __syncthreads();
  if (o == 0) {
    double ta = 0.0, tc = 0.0;
    for (int k = 0; k < outSteps; ++k) { ta += hAbs[k]; tc += hCnt[k]; }
    result[0] = tc > 0.0 ? (float)(ta / tc) : 0.f;      // all-masked: mask/mean(mask) is nan -> 0 (loss.py:24-27)
    const_cast<float*>(partials)[2 * B * outSteps] = (float)tc;   // kept for the gradient (k_mae_grad)
  }
}

// ---- the evaluator's metric table (traffic_state_evaluator.py:46-121; group-std re-transform of
// traffic_state_executor.py:293-322) ---------------------------------------------------------------------------------
// One pass over prediction and label gives, per horizon, the MATGCN_METRIC_SUMS sums every metric of the table is a
// ratio of; they are accumulated in fp64 (R2 / EVAR subtract squares of means).  Element-wise arithmetic is fp32, like
// the reference's tensors.  stage 1: one workgroup per (b, horizon) -> partials[b][o][.]; stage 2 adds the batch up
// in a fixed order (run-to-run identical) and, on request, onto the running sums of earlier batches.
struct MetricArgs {
  // the argument order from before LabelView and NodeScale, whose fields these are (both metric kernels measured slower
  // with the two blocks embedded: DESIGN.md 5f)
  const float* pred;     // (B, out, N, od)
  const float* y;        // (B, ySteps, N, yFeat) windows, or the raw series (ySteps, N, yFeat) when labelStart != null
  const int* labelStart;
  const float* mean; const float* std;     // first affine x*std + mean: one value, or N values (perNode); null = identity
  const float* mean2; const float* std2;   // second affine, per node (the group-std re-transform), or null
  int perNode;
  float clampMin;        // prediction below -> clampMin (NaN: off)
  float truthMin;        // only elements whose label exceeds it take part (NaN: off)
  float minS;            // |label| < minS -> 0 (loss.py:18; < 0: off)
  int outSteps, N, od, ySteps, yFeat, yStart;
  double* partials;      // [B*out][MATGCN_METRIC_SUMS]
};
__device__ __forceinline__ LabelView metric_labels(const MetricArgs& a) {
  return {a.y, a.labelStart, a.outSteps, a.N, a.od, a.ySteps, a.yFeat, a.yStart};
}
constexpr int METRIC_SUMS = 14;
// sums: 0 elements, 1 non-NaN labels, 2 |d|, 3 d^2, 4 |d/l| (over 1), 5 labels != 0, 6-8 the same three over 5,
//       9 l, 10 l^2, 11 p, 12 p^2, 13 l-p
// The terms of one element - raw label l and prediction p of node n - added onto s[], one add per sum: both groupings
// of the sums (per horizon, per horizon and node) are this function, so their per-element terms cannot differ.
__device__ __forceinline__ void metric_add_element(const MetricArgs& a, bool clamp, bool pick, int n, float l, float p,
                                                   double* s) {
  // descale_node's statements, kept here for the pair: two calls of it cost k_metric_partial four VGPRs (44 -> 48)
  if (a.std) {
    const float sd = a.std[a.perNode ? n : 0], mu = a.mean[a.perNode ? n : 0];
    l = scale_affine(l, sd, mu); p = scale_affine(p, sd, mu);
  }
  if (a.std2) { l = scale_affine(l, a.std2[n], a.mean2[n]); p = scale_affine(p, a.std2[n], a.mean2[n]); }
  if (clamp && p < a.clampMin) p = a.clampMin;
  if (pick && !(l > a.truthMin)) return;
  if (a.minS >= 0.f && fabsf(l) < a.minS) l = 0.f;
  const float d = p - l, ad = fabsf(d), sq = d * d, ap = fabsf(d / l);
  const bool valid = l == l, nz = l != 0.f;          // NaN != 0 holds, as in labels.ne(0)
  s[0] += 1.0;
  if (valid) { s[1] += 1.0; s[2] += ad == ad ? ad : 0.f; s[3] += sq == sq ? sq : 0.f; s[4] += ap == ap ? ap : 0.f; }
  if (nz) { s[5] += 1.0; s[6] += ad == ad ? ad : 0.f; s[7] += sq == sq ? sq : 0.f; s[8] += ap == ap ? ap : 0.f; }
  const double ld = l, pd = p;
  s[9] += ld; s[10] += ld * ld; s[11] += pd; s[12] += pd * pd; s[13] += ld - pd;
}

__global__ __launch_bounds__(256) void k_metric_partial(MetricArgs a) {
  __shared__ double red[4][METRIC_SUMS];
  const LabelView v = metric_labels(a);
  const int b = blockIdx.x / v.outSteps, o = blockIdx.x - b * v.outSteps;
  const float* pp = a.pred + ((size_t)b * v.outSteps + o) * v.N * v.od;
  const float* yp = label_ptr(v, label_row(v, b, o), 0);
  double s[METRIC_SUMS];
#pragma unroll
  for (int k = 0; k < METRIC_SUMS; ++k) s[k] = 0.0;
  const bool clamp = a.clampMin == a.clampMin, pick = a.truthMin == a.truthMin;
  for (int idx = threadIdx.x; idx < v.N * v.od; idx += 256) {
    const int n = idx / v.od, c = idx - n * v.od;
    metric_add_element(a, clamp, pick, n, yp[(size_t)n * v.yFeat + c], pp[idx], s);
  }
#pragma unroll
  for (int k = 0; k < METRIC_SUMS; ++k) {
    double v = s[k];
    for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_down(v, sh, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < METRIC_SUMS)
    a.partials[(size_t)blockIdx.x * METRIC_SUMS + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// stage 2: block o, thread k: sums[o][k] (+)= sum_b partials[b][o][k]
__global__ __launch_bounds__(64) void k_metric_accumulate(const double* __restrict__ partials, int B, int outSteps,
                                                          int accumulate, double* __restrict__ sums) {
  const int o = blockIdx.x, k = threadIdx.x;
  if (k >= METRIC_SUMS) return;
  double v = 0.0;
  for (int b = 0; b < B; ++b) v += partials[((size_t)b * outSteps + o) * METRIC_SUMS + k];
  sums[o * METRIC_SUMS + k] = (accumulate ? sums[o * METRIC_SUMS + k] : 0.0) + v;
}

// The same sums grouped per (horizon, node): thread (o, n) walks the batch itself and adds the terms of its elements one
// at a time in ascending (b, c), onto the stored sums when accumulate is set - the value is a chain of adds in an order
// the data alone fixes, so one call over B rows and accumulating calls over the same rows in pieces give the same bits.
// No scratch, no second stage; lanes of a wave hold consecutive nodes of one horizon (coalesced for od = 1).
__global__ __launch_bounds__(64) void k_metric_nodes(MetricArgs a, int B, int accumulate, double* __restrict__ sums) {
  const LabelView v = metric_labels(a);
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= v.outSteps * v.N) return;
  const int o = idx / v.N, n = idx - o * v.N;
  double s[METRIC_SUMS];
#pragma unroll
  for (int k = 0; k < METRIC_SUMS; ++k) s[k] = accumulate ? sums[(size_t)idx * METRIC_SUMS + k] : 0.0;
  const bool clamp = a.clampMin == a.clampMin, pick = a.truthMin == a.truthMin;
  for (int b = 0; b < B; ++b) {
    const float* yp = label_ptr(v, label_row(v, b, o), n);
    const float* pp = a.pred + (((size_t)b * v.outSteps + o) * v.N + n) * v.od;
    for (int c = 0; c < v.od; ++c) metric_add_element(a, clamp, pick, n, yp[c], pp[c], s);
  }
#pragma unroll
  for (int k = 0; k < METRIC_SUMS; ++k) sums[(size_t)idx * METRIC_SUMS + k] = s[k];
}

// one row of the table from its 14 sums; m: MAE, MAPE, MSE, RMSE, masked_MAE, masked_MAPE, masked_MSE, masked_RMSE, R2,
// EVAR (the order of TrafficStateEvaluator.json).  swap: R2 / EVAR with prediction and truth exchanged, as
// traffic_state_executor.py:318-319 hands them to sklearn.
__device__ __forceinline__ void metric_row(const double* s, int swap, double* t) {
  const double n = s[0];
  // mask / mean(mask) then mean: sum over the kept elements / their count; nothing kept -> nan -> 0 (loss.py:24-27)
  t[0] = s[1] > 0 ? s[2] / s[1] : 0.0;
  t[1] = s[1] > 0 ? s[4] / s[1] : 0.0;
  t[2] = s[1] > 0 ? s[3] / s[1] : 0.0;
  t[3] = sqrt(t[2]);
  t[4] = s[5] > 0 ? s[6] / s[5] : 0.0;
  t[5] = s[5] > 0 ? s[8] / s[5] : 0.0;
  t[6] = s[5] > 0 ? s[7] / s[5] : 0.0;
  t[7] = sqrt(t[6]);
  // sklearn r2_score(y_true, y_pred) = 1 - sum (t-p)^2 / sum (t - mean t)^2, explained_variance_score = 1 - Var(t-p)/Var(t)
  // (the residual sum leaves NaN labels out; sklearn refuses such input anyway)
  const double s1 = swap ? s[11] : s[9], s2 = swap ? s[12] : s[10];
  const double ssTot = n > 0 ? s2 - s1 * s1 / n : 0.0, res = s[3];
  const double varD = n > 0 ? res / n - (s[13] / n) * (s[13] / n) : 0.0;
  const double varT = n > 0 ? ssTot / n : 0.0;
  t[8] = ssTot != 0.0 ? 1.0 - res / ssTot : (res == 0.0 ? 1.0 : 0.0);
  t[9] = varT != 0.0 ? 1.0 - varD / varT : (varD == 0.0 ? 1.0 : 0.0);
}

// table[mode][o][m]: mode 0 "single" = horizon o alone, mode 1 "average" = horizons 0..o (traffic_state_evaluator.py:
// 46-121); columns as metric_row.
__global__ __launch_bounds__(64) void k_metric_table(const double* __restrict__ sums, int outSteps, int swap,
                                                     double* __restrict__ table) {
  const int o = threadIdx.x;
  if (o >= outSteps) return;
  for (int mode = 0; mode < 2; ++mode) {
    double s[METRIC_SUMS];
    for (int k = 0; k < METRIC_SUMS; ++k) s[k] = 0.0;
    for (int q = mode ? 0 : o; q <= o; ++q)
      for (int k = 0; k < METRIC_SUMS; ++k) s[k] += sums[q * METRIC_SUMS + k];
    metric_row(s, swap, table + ((size_t)mode * outSteps + o) * 10);
  }
}

// table[r][m] from sum_{f < fold} sums[f * rows + r][.], added in ascending f from 0 - with fold = 1 the arithmetic of
// k_metric_table's "single" mode, add of the zero included
__global__ __launch_bounds__(256) void k_metric_table_rows(const double* __restrict__ sums, int rows, int fold, int swap,
                                                           double* __restrict__ table) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  double s[METRIC_SUMS];
  for (int k = 0; k < METRIC_SUMS; ++k) s[k] = 0.0;
  for (int f = 0; f < fold; ++f)
    for (int k = 0; k < METRIC_SUMS; ++k) s[k] += sums[((size_t)f * rows + r) * METRIC_SUMS + k];
  metric_row(s, swap, table + (size_t)r * 10);
}

// gradient of result[0] w.r.t. pred: upstream * std * sign(p - l) * mask / sum(mask)   (torch: d|x| = sign(x), 0 at 0;
// terms the forward replaced by 0 - NaN differences - get no gradient)
__global__ __launch_bounds__(256) void k_mae_grad(const float* __restrict__ pred, const float* __restrict__ y,
                                                  const int* __restrict__ labelStart, int outSteps, int N, int od,
                                                  int ySteps, int yFeat, int yStart, float mean, float std,
                                                  float nullVal, float minS,
                                                  const float* __restrict__ count, const float* __restrict__ upstream,
                                                  size_t total, float* __restrict__ dpred) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = idx % od;
  const int n = (idx / od) % N;
  const int o = (idx / ((size_t)od * N)) % outSteps;
  const size_t b = idx / ((size_t)od * N * outSteps);
  const size_t yrow = labelStart ? series_row((long)labelStart[b] + o, ySteps) : b * ySteps + o;
  float l = y[(yrow * N + n) * yFeat + yStart + c] * std + mean;
  const float p = pred[idx] * std + mean;
  if (fabsf(l) < minS) l = 0.f;
  const bool nanMask = nullVal != nullVal;
  const float m = nanMask ? (l == l ? 1.f : 0.f) : (l != nullVal ? 1.f : 0.f);
  const float d = p - l;
  const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);      // NaN compares false both ways: 0
  const float cnt = count[0];
  dpred[idx] = cnt > 0.f ? upstream[0] * std * sgn * m / cnt : 0.f;
}

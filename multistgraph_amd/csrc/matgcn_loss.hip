// matgcn_loss.hip - the executor's differentiable training objectives on the device, value and gradient (matgcn_loss /
// matgcn_loss_grad, include/matgcn.h): mae, mse, rmse, mape (loss.masked_*_torch, libcity/model/loss.py:17-90), logcosh,
// huber, quantile (loss.py:32-51), as TrafficStateExecutor._build_train_loss picks them (traffic_state_executor.py:200-250).
// Included by matgcn_capi.hip.  One kernel family, the kind a template parameter: the element loop has no runtime switch.
//
// Geometry is that of section 9 of matgcn_kernels.hip (k_mae_partial): pred (B, out, N, od); y (B, ySteps, N, yFeat) channels
// yStart .., or with labelStart the raw series (ySteps, N, yFeat) gathered through series_row (clamped and counted).
//
// Arithmetic.  l = y*std + mean and p = pred*std + mean are two fp32 roundings each (scale_affine), and d = p - l one more:
// the values the reference's float32 tensors hold.  From there on everything is fp64 - the term of an element, the sums, the
// quotient, the square root - and a result is rounded to float32 ONCE.  The partials of stage 1 are doubles.
//   MASKED (MAE, MSE, RMSE, MAPE):  l := 0 where |l| < minS first; m = (l != nullVal) [nullVal NaN: !isnan(l)];
//     value = sum(t*m) / sum(m).  A term that is NaN after masking adds 0 and gets gradient 0 (it still counts in sum(m),
//     as in k_mae_partial / loss.py:27-29); an infinite one stays infinite (MAPE on an unmasked zero label); nothing kept: 0.
//   not MASKED (LOGCOSH, HUBER, QUANTILE): the plain mean over all B*out*N*od elements; a NaN label makes the value NaN.
// LOGCOSH is |d| + log1p(exp(-2|d|)) - ln 2, not log(cosh(d)): the reference's form overflows to inf in float32 once |d|
// passes about 89, which de-scaled visit counts do routinely.  This is the one deliberate departure from the reference's
// float32 bits.  RMSE: the gradient is d / rmse * ...; where rmse == 0 every gradient is 0 (torch gives NaN there: 0/0).
//
// Order.  Stage 1: one workgroup of 256 per (b, horizon) slab; thread t adds the elements t, t + 256, .. in ascending index,
// the 64 lanes of a wave fold by halves, thread 0 adds the four waves in ascending order.  Stage 2: one workgroup; thread o
// adds horizon o over the batch in ascending b, thread 0 the horizons in ascending order.  No atomics: two calls give the same
// bits.  scratch: 2*B*out doubles (term sum, count per slab), then 2 more that stage 2 leaves for the gradient: the count
// over all horizons and, for RMSE, the fp64 mse.  Every word of it that is read is written first by the same call.

constexpr int LOSS_THREADS = 256;

__device__ __forceinline__ double loss_sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }   // NaN: 0

// the term of one element from the fp32 values p, l and d = p - l
template <int KIND>
__device__ __forceinline__ double loss_term(float pf, float lf, float df, double delta) {
  const double d = (double)df;
  if (KIND == MATGCN_LOSS_MAE) return fabs(d);
  if (KIND == MATGCN_LOSS_MSE || KIND == MATGCN_LOSS_RMSE) return d * d;
  if (KIND == MATGCN_LOSS_MAPE) return fabs(d / (double)lf);
  if (KIND == MATGCN_LOSS_LOGCOSH) {
    const double a = fabs(d);
    return a + log1p(exp(-2.0 * a)) - 0.69314718055994530942;
  }
  if (KIND == MATGCN_LOSS_HUBER) {
    const double a = fabs(d);
    return a <= delta ? 0.5 * a * a : delta * a - 0.5 * delta * delta;
  }
  return lf >= pf ? delta * -d : (1.0 - delta) * d;      // QUANTILE; a NaN label fails l >= p and p - l carries it on
}

// d term / d p (RMSE: of the mse term; k_loss_grad divides by 2 rmse)
template <int KIND>
__device__ __forceinline__ double loss_slope(float pf, float lf, float df, double delta) {
  const double d = (double)df;
  if (KIND == MATGCN_LOSS_MAE) return loss_sign(d);
  if (KIND == MATGCN_LOSS_MSE || KIND == MATGCN_LOSS_RMSE) return 2.0 * d;
  if (KIND == MATGCN_LOSS_MAPE) return loss_sign(d) / fabs((double)lf);
  if (KIND == MATGCN_LOSS_LOGCOSH) return tanh(d);
  if (KIND == MATGCN_LOSS_HUBER) return fabs(d) <= delta ? d : delta * loss_sign(d);
  return lf >= pf ? -delta : 1.0 - delta;
}

struct LossArgs {
  const float* pred;
  LabelView lab;
  float mean, std, nullVal, minS, delta;
};

// p, l, d of one element and whether the mask keeps it
template <int MASKED>
__device__ __forceinline__ bool loss_element(const LossArgs& a, float yv, float pv, float& p, float& l, float& d) {
  l = scale_affine(yv, a.std, a.mean);
  p = scale_affine(pv, a.std, a.mean);
  bool keep = true;
  if (MASKED) {
    if (fabsf(l) < a.minS) l = 0.f;                       // loss.py:18/55/73/88 (in place in the reference)
    keep = (a.nullVal != a.nullVal) ? (l == l) : (l != a.nullVal);
  }
  d = p - l;
  return keep;
}

// stage 1: scratch[2 * slab] = sum of the kept terms of slab (b, o), scratch[2 * slab + 1] = the kept elements
template <int KIND, int MASKED>
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_partial(LossArgs a, double* __restrict__ scratch) {
  __shared__ double red[LOSS_THREADS / 64][2];
  const LabelView& v = a.lab;
  const int b = blockIdx.x / v.outSteps, o = blockIdx.x - b * v.outSteps;
  const int len = v.N * v.od;
  const float* pp = a.pred + ((size_t)b * v.outSteps + o) * len;
  const float* yp = label_ptr(v, label_row(v, b, o), 0);
  const double delta = (double)a.delta;
  double st = 0.0, sc = 0.0;
  for (int idx = threadIdx.x; idx < len; idx += LOSS_THREADS) {
    const int n = idx / v.od, c = idx - n * v.od;
    float p, l, d;
    const bool keep = loss_element<MASKED>(a, yp[(size_t)n * v.yFeat + c], pp[idx], p, l, d);
    const double t = loss_term<KIND>(p, l, d, delta);
    if (MASKED) {
      if (keep) { sc += 1.0; st += (t == t) ? t : 0.0; }
    } else {
      sc += 1.0; st += t;
    }
  }
  for (int sh = 32; sh > 0; sh >>= 1) { st += __shfl_down(st, sh, 64); sc += __shfl_down(sc, sh, 64); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = st; red[threadIdx.x >> 6][1] = sc; }
  __syncthreads();
  if (threadIdx.x < 2)
    scratch[2 * (size_t)blockIdx.x + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

template <int KIND>
__device__ __forceinline__ double loss_value(double sum, double cnt) {
  const double v = cnt > 0.0 ? sum / cnt : 0.0;           // nothing kept: mask / mean(mask) is NaN -> 0 (loss.py:24-25)
  return KIND == MATGCN_LOSS_RMSE ? sqrt(v) : v;
}

// stage 2: result[0] over all horizons, result[1 + k] horizon k alone; scratch[2 B out] = count, [2 B out + 1] = fp64 mse
template <int KIND>
__global__ __launch_bounds__(64) void k_loss_final(double* __restrict__ scratch, int B, int outSteps,
                                                   float* __restrict__ result) {
  __shared__ double hSum[64], hCnt[64];
  const int o = threadIdx.x;
  double st = 0.0, sc = 0.0;
  if (o < outSteps)
    for (int b = 0; b < B; ++b) {
      st += scratch[2 * ((size_t)b * outSteps + o)];
      sc += scratch[2 * ((size_t)b * outSteps + o) + 1];
    }
  hSum[o] = st; hCnt[o] = sc;
  if (o < outSteps) result[1 + o] = (float)loss_value<KIND>(st, sc);
  __syncthreads();
  if (o == 0) {
    double ts = 0.0, tc = 0.0;
    for (int k = 0; k < outSteps; ++k) { ts += hSum[k]; tc += hCnt[k]; }
    result[0] = (float)loss_value<KIND>(ts, tc);
    scratch[2 * (size_t)B * outSteps] = tc;
    scratch[2 * (size_t)B * outSteps + 1] = tc > 0.0 ? ts / tc : 0.0;
  }
}

// d result[0] / d pred: upstream * std * g * m / count, formed in fp64 and rounded once; one thread per element
template <int KIND, int MASKED>
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_grad(LossArgs a, const double* __restrict__ kept,
                                                            const float* __restrict__ upstream, size_t total,
                                                            float* __restrict__ dpred) {
  const size_t idx = (size_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
  if (idx >= total) return;
  const LabelView& v = a.lab;
  const int c = idx % v.od;
  const int n = (idx / v.od) % v.N;
  const int o = (idx / ((size_t)v.od * v.N)) % v.outSteps;
  const size_t b = idx / ((size_t)v.od * v.N * v.outSteps);
  float p, l, d;
  const bool keep = loss_element<MASKED>(a, label_at(v, label_row(v, b, o), n, c), a.pred[idx], p, l, d);
  const double delta = (double)a.delta;
  const double cnt = MASKED ? kept[0] : (double)total;
  double g = 0.0;
  if (keep && cnt > 0.0) {
    g = loss_slope<KIND>(p, l, d, delta);
    if (MASKED) {
      const double t = loss_term<KIND>(p, l, d, delta);
      if (t != t) g = 0.0;                                // the forward replaced this term by 0
    }
    if (KIND == MATGCN_LOSS_RMSE) {
      const double rmse = sqrt(kept[1]);
      g = rmse > 0.0 ? g / (2.0 * rmse) : 0.0;            // rmse == 0: torch's 0 / 0; no direction to move in, 0 here
    }
    g = (double)upstream[0] * (double)a.std * g / cnt;
  }
  dpred[idx] = (float)g;
}

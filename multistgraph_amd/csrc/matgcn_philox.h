// matgcn_philox.h - the counter-based generator behind the device-side dropout (matgcn_dropout, include/matgcn.h).
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123): ten
// rounds of two 32 x 32 -> 64-bit products, multipliers 0xD2511F53 / 0xCD9E8D57, key bumped by the Weyl constants
// 0x9E3779B9 / 0xBB67AE85 between rounds.  No state: the four output words are a function of (counter, key) alone, so
// every kernel that needs a dropout decision recomputes it from the element's position and no mask lives in memory.
//
// The dropout in front of end_conv (MultiATGCN.py:416) over the logical (B, headT, N, 64) mask:
//   idx     = ((b * headT + t') * N + n) * 64 + h          the element's position (independent of Np, tiles, schedule)
//   key     = (lo32(seed), hi32(seed))
//   counter = (lo32(idx >> 2), hi32(idx >> 2), lo32(offset), hi32(offset))
//   element idx is kept iff output word (idx & 3) >= thr,  thr = floor((double)p * 2^32)
//   multiplier = keep ? (float)(1 / (1 - (double)p)) : 0
// One call decides four consecutive hidden channels - the float4 a lane of every site handles.
#ifndef MATGCN_PHILOX_H
#define MATGCN_PHILOX_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MATGCN_HD __host__ __device__ __forceinline__
#else
#define MATGCN_HD inline
#endif

// kernel-side form of matgcn_dropout (make_drop_desc, matgcn_capi.hip); on == 0: no descriptor
struct DropDesc {
  unsigned long long seed;
  unsigned long long offset;
  unsigned int thr;      // keep iff word >= thr
  float scale;           // multiplier of a kept element
  int on;
  int pad_;
};

struct Philox4 { uint32_t w[4]; };

MATGCN_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the four output words of mask quad q = idx >> 2
MATGCN_HD Philox4 drop_words(const DropDesc& d, unsigned long long q) {
  return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)d.offset, (uint32_t)(d.offset >> 32), (uint32_t)d.seed,
                       (uint32_t)(d.seed >> 32));
}

// bit i set: element 4 q + i is kept
MATGCN_HD unsigned int drop_keep4(const DropDesc& d, unsigned long long q) {
  const Philox4 x = drop_words(d, q);
  return (x.w[0] >= d.thr ? 1u : 0u) | (x.w[1] >= d.thr ? 2u : 0u) | (x.w[2] >= d.thr ? 4u : 0u) |
         (x.w[3] >= d.thr ? 8u : 0u);
}

#if defined(__HIPCC__) || defined(__CUDACC__)
// the four multipliers of mask quad q
__device__ __forceinline__ float4 drop_mult4(const DropDesc& d, unsigned long long q) {
  const Philox4 x = drop_words(d, q);
  return make_float4(x.w[0] >= d.thr ? d.scale : 0.f, x.w[1] >= d.thr ? d.scale : 0.f, x.w[2] >= d.thr ? d.scale : 0.f,
                     x.w[3] >= d.thr ? d.scale : 0.f);
}
#endif

#endif

// Standard-normal draws of the kernels that take noise: the tensor the caller passed, or a counter-based generator.
// Included by every kernel that draws (sched.hip, ilvr.hip, elementwise.hip): ONE definition, so that a draw is the same
// number whichever kernel makes it. philox_normal switches fp contraction off for its own body only, and takes its logarithm
// from the builtin at that place: the compiler expands it into log2(x) times ln 2 in two parts, and under contraction - which
// the header's __logf wrapper inherits from the including file - it fuses the last add of that expansion and gives another last
// bit (the copy elementwise.hip once had did). The including file's own arithmetic keeps its setting.
#pragma once
#include "common.h"
#include "kernels.h"

namespace cd {

// ---------------- counter-based RNG (Philox4x32-10 + Box-Muller) for throughput runs ----------
__device__ inline void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ inline float philox_normal(uint64_t seed, uint32_t stream, uint64_t idx) {
#pragma clang fp contract(off)
  // one normal per (stream, idx): counter = (idx/2, stream), Box-Muller pair selected by idx&1
  uint32_t c[4] = {(uint32_t)(idx >> 1), (uint32_t)(idx >> 33), stream, 0x9E3779B9u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  float u1 = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  float u2 = ((float)(c[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  float rad = sqrtf(-2.0f * __builtin_logf(u1));  // what __logf returns, with this body's contraction setting
  float ang = 6.28318530717958647692f * u2;
  return (idx & 1) ? rad * __sinf(ang) : rad * __cosf(ang);
}

__device__ inline float draw(const GaussSrc& g, int64_t i) {
  return g.noise ? g.noise[i] : philox_normal(g.seed, g.stream, (uint64_t)i);
}

}  // namespace cd

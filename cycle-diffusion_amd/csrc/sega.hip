// Semantic guidance (SEGA; Brack et al., NeurIPS 2023) on the decoder rows of the coupled loop: between the
// forward and the unchanged decode step kernel, two launches turn the network's outputs of the row's unconditional,
// conditional and E concept rows into the eps the step consumes.
//
//   d_e   = (p_e - u) * s_e ;  a_e = |d_e|
//   tau_e = A[lo_e] + (A[hi_e] - A[lo_e]) * frac_e        A = a_e[r, .] ascending, hi = min(lo + 1, N - 1)   k_sega_threshold
//   m_e   = (a_e >= tau_e) ? d_e : 0
//   gamma = ((0 + w_0*m_0) + w_1*m_1) + ...               active concepts, ascending e                       k_sega_combine
//   gamma'= gamma + s_m * nu ;  nu <- beta*nu + (1 - beta)*gamma' ;  eps = (u + g*(c - u)) + gamma'
//
// fp32 in the operation order written above, contraction off (build.py), as sched.hip keeps it: tests/_sega_ref.py restates
// the same order in torch and the op test compares bit for bit. There is no counterpart in the reference tree.
#include "common.h"
#include "kernels.h"
#include "sched_elem.h"

namespace cd {

#pragma clang fp contract(off)

namespace {

constexpr int kSegaThreads = 256;  // four waves: the histogram has one bin per thread

// index of the n-th set bit of m (n < popcount(m)): block y of the threshold grid -> its concept
__device__ inline int nth_set_bit(uint32_t m, int n) {
  for (int i = 0; i < n; ++i) m &= m - 1;
  return __ffs((int)m) - 1;
}

// sum / minimum over the workgroup; every thread gets the result. red: kSegaThreads / 64 words of LDS.
__device__ inline unsigned block_sum(unsigned v, unsigned* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();  // red may still be read from the reduction before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ inline unsigned block_min(unsigned v, unsigned* red) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_down(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return min(min(red[0], red[1]), min(red[2], red[3]));
}

// One workgroup per (decoder row r, concept e active in this iteration). a = |d| >= 0, so the unsigned order of the bit
// patterns is the order of the floats (a NaN, whatever its payload, sorts above +inf: a row that holds one has it as its
// largest values, and a tau computed from it is NaN, which keeps nothing). Radix selection of the rank-lo value: four 8-bit
// passes from the top byte, each a 256-bin LDS histogram of the values that share the prefix found so far and a one-wave scan
// for the bin that holds the rank. The last pass leaves the bit pattern of A[lo], the rank inside its run of equal values and
// the run's length: A[hi] is the same value if rank lo + 1 is still inside the run, else the smallest value above it.
// a is written once to a.abuf [Bd*E][N] (thread t owns elements t, t + 256, ...: every re-read is of the thread's own
// stores) and re-read by the later passes; one code path for every N.
__global__ __launch_bounds__(kSegaThreads) void k_sega_threshold(SegaStep a) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sel[3];  // the bin that holds the rank, the rank inside it, its count
  __shared__ unsigned red[kSegaThreads / 64];
  const int r = blockIdx.x, e = nth_set_bit(a.active, blockIdx.y);
  const int N = a.C * a.HW, tid = threadIdx.x;
  const SegaConcept cp = a.tab[e];
  float* A = a.abuf + ((int64_t)r * a.E + e) * N;
  const float* pu = a.eh.p + (int64_t)r * a.eh.sb;
  const float* pe = a.eh.p + ((int64_t)(1 + e) * a.Bd + r) * a.eh.sb;

  unsigned prefix = 0, rank = (unsigned)cp.lo, run = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
    hist[tid] = 0;
    __syncthreads();
    for (int j = tid; j < N; j += kSegaThreads) {
      float av;
      if (pass == 0) {
        const int c = j / a.HW, p = j - c * a.HW;
        const int64_t at = (int64_t)c * a.eh.sc + (int64_t)p * a.eh.sp;
        const float d = (pe[at] - pu[at]) * cp.scale;
        av = fabsf(d);
        A[j] = av;
      } else {
        av = A[j];
      }
      const unsigned bits = __float_as_uint(av);
      if ((bits & himask) == prefix) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {
      const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const unsigned s = c0 + c1 + c2 + c3;
      unsigned incl = s;
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (tid >= o) incl += up;
      }
      unsigned ex = incl - s;  // values in the bins below this lane's four
      if (rank >= ex && rank < ex + s) {
        unsigned bin = 4 * tid, cnt = c0;
        if (rank >= ex + c0) { ex += c0; bin += 1; cnt = c1;
          if (rank >= ex + c1) { ex += c1; bin += 1; cnt = c2;
            if (rank >= ex + c2) { ex += c2; bin += 1; cnt = c3; } } }
        sel[0] = bin; sel[1] = rank - ex; sel[2] = cnt;
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    rank = sel[1];
    run = sel[2];
    __syncthreads();  // sel and hist are rewritten by the next pass
  }
  const float a_lo = __uint_as_float(prefix);
  float a_hi = a_lo;
  if (cp.lo + 1 <= N - 1 && rank + 1 >= run) {  // rank lo + 1 lies past the run of values equal to A[lo]
    unsigned mn = 0xFFFFFFFFu;
    for (int j = tid; j < N; j += kSegaThreads) {
      const unsigned bits = __float_as_uint(A[j]);
      if (bits > prefix) mn = min(mn, bits);
    }
    a_hi = __uint_as_float(block_min(mn, red));
  }
  const float diff = a_hi - a_lo;
  const float step = diff * cp.frac;
  const float tau = a_lo + step;
  unsigned n_kept = 0;
  for (int j = tid; j < N; j += kSegaThreads) n_kept += (A[j] >= tau) ? 1u : 0u;
  n_kept = block_sum(n_kept, red);
  if (tid == 0) {
    a.tau[(int64_t)r * a.E + e] = tau;
    a.kept[(int64_t)r * a.E + e] = (int)n_kept;
  }
}

// eps and nu of every element of the Bd decoder rows from u, c, the active p_e and their tau; d_e is formed again by the
// expression k_sega_threshold formed it by, so a_e >= tau_e here is the comparison its kept count made.
__global__ void k_sega_combine(SegaStep a) {
  StepGeom g;
  g.B = a.Bd; g.C = a.C; g.HW = a.HW;
  const int64_t chw = (int64_t)a.C * a.HW;
  const float omb = 1.f - a.beta;
  for_each_elem(g, [&](const Elem& el) {
    const float u = eps_hat_at(a.eh, el.b, el);
    const float c = eps_hat_at(a.eh, el.b + (1 + a.E) * a.Bd, el);
    const float gs = a.eh.gvec ? a.eh.gvec[el.b] : a.eh.g;
    const float base = u + gs * (c - u);  // load_eps_hat's expression
    float gamma = 0.f;
    for (int e = 0; e < a.E; ++e) {
      float keep = 0.f;
      if ((a.active >> e) & 1u) {
        const SegaConcept cp = a.tab[e];
        const float p = eps_hat_at(a.eh, el.b + (1 + e) * a.Bd, el);
        const float d = (p - u) * cp.scale;
        const float av = fabsf(d);
        float m = 0.f;
        if (av >= a.tau[(int64_t)el.b * a.E + e]) { m = d; keep = 1.f; }
        const float wm = cp.weight * m;
        gamma = gamma + wm;
      }
      if (a.mask_out) a.mask_out[((int64_t)el.b * a.E + e) * chw + el.rem] = keep;
    }
    const float nu = a.nu[el.i];
    const float mom = a.s_m * nu;
    const float gp = gamma + mom;
    const float n0 = a.beta * nu;
    const float n1 = omb * gp;
    a.nu[el.i] = n0 + n1;
    a.eps[el.i] = base + gp;
  });
}

}  // namespace

void launch_sega_guidance(hipStream_t st, const SegaStep& a) {
  const int n_active = __builtin_popcount(a.active);
  if (n_active)
    hipLaunchKernelGGL(k_sega_threshold, dim3((unsigned)a.Bd, (unsigned)n_active), dim3(kSegaThreads), 0, st, a);
  StepGeom g;
  g.B = a.Bd; g.C = a.C; g.HW = a.HW;
  hipLaunchKernelGGL(k_sega_combine, ew_grid(g), dim3(256), 0, st, a);
}

}  // namespace cd

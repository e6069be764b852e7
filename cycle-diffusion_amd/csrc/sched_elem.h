// The element loop and the network-output view that the per-step kernels of sched.hip and sega.hip share.
#pragma once
#include "common.h"
#include "kernels.h"

namespace cd {

// element i = b*C*HW + rem of an NCHW tensor, rem = c*HW + p
struct Elem {
  int64_t i, rem;
  int b, c, p;
};

// grid-stride loop over the B*C*HW elements
template <class F>
__device__ inline void for_each_elem(const StepGeom& g, F f) {
  const int64_t chw = (int64_t)g.C * g.HW, n = (int64_t)g.B * chw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    Elem e;
    e.i = i;
    e.b = (int)(i / chw);
    e.rem = i - (int64_t)e.b * chw;
    e.c = (int)(e.rem / g.HW);
    e.p = (int)(e.rem - (int64_t)e.c * g.HW);
    f(e);
  }
}

__device__ inline float eps_hat_at(const EpsHat& eh, int b, const Elem& e) {
  return eh.p[(int64_t)b * eh.sb + (int64_t)e.c * eh.sc + (int64_t)e.p * eh.sp];
}

static inline dim3 ew_grid(const StepGeom& g) {
  int64_t n = ((int64_t)g.B * g.C * g.HW + 255) / 256;
  return dim3((unsigned)(n > 2048 ? 2048 : (n < 1 ? 1 : n)));
}

}  // namespace cd

// Fused windows on the coupled loop (MultiDiffusion, Bar-Tal et al. 2023): the running latent lives on a canvas
// [Hc, Wc] larger than the network's S x S input, the network runs on n_win overlapping S x S windows of it as more batch
// rows of the one forward, and the noise prediction of a canvas cell is the average of the windows that cover it.
//   k_window_gather  canvas fp32 NCHW -> the windows' network input rows, 16-bit NHWC (what launch_nchw_to_nhwc writes of a
//                    network-sized latent)
//   k_window_fuse    the windows' network output rows fp32 NHWC -> canvas fp32 NCHW, per-cell average in ascending window order
// Both are memory-bound passes over a few hundred KB per row. No atomics: every output element has one owner that gathers.
#include "common.h"
#include "kernels.h"

namespace cd {

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

inline dim3 win_grid(int64_t n) {
  const int64_t g = (n + kThreads - 1) / kThreads;
  return dim3((unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g)));
}

// the window offsets (y, x) of the call, once per block
__device__ inline void load_offsets(const int* __restrict__ win, int n_win, int* s_win) {
  for (int i = threadIdx.x; i < 2 * n_win; i += blockDim.x) s_win[i] = win[i];
  __syncthreads();
}

// One item = 8 channels (16 B) of one pixel of one output row: a wave's 64 stores are one contiguous KiB. Only the items that
// hold real channels read; at C = 4, cpad = 32 that is every fourth lane, and neighbouring pixels' reads share their lines.
__global__ void __launch_bounds__(kThreads) k_window_gather(WindowGather a) {
  __shared__ int s_win[2 * kMaxWindows];
  load_offsets(a.win, a.n_win, s_win);
  const int nv = a.cpad / 8, SS = a.S * a.S;
  const int64_t per_part = (int64_t)a.n_win * a.Bp * SS * nv;  // items of one part; the parts repeat it
  const int64_t plane = (int64_t)a.Hc * a.Wc;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per_part; i += (int64_t)gridDim.x * blockDim.x) {
    const int v = (int)(i % nv);
    const int64_t rp = i / nv;
    const int pix = (int)(rp % SS);
    const int row = (int)(rp / SS);  // w * Bp + b
    const int w = row / a.Bp, b = row - w * a.Bp;
    const int y = s_win[2 * w] + pix / a.S, x = s_win[2 * w + 1] + pix % a.S;
    const float* src = a.x + (int64_t)b * a.C * plane + (int64_t)y * a.Wc + x;
    uint32_t h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 8 * v + j;
      h[j] = c < a.C ? (uint32_t)f2bf(src[(int64_t)c * plane]) : (uint32_t)f2bf(0.f);
    }
    const uint4 out = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    for (int d = 0; d <= a.dup; ++d) *(uint4*)(a.y + (d * per_part + i) * 8) = out;
  }
}

// the count and the sum of the windows over cell (y, x), ascending w, the first one without an add: `load(w)` reads the cell's
// value in window w
template <class F>
__device__ inline float fuse_cell(const int* s_win, int n_win, int S, int y, int x, F load) {
  float acc = 0.f;
  int count = 0;
  for (int w = 0; w < n_win; ++w) {
    const int wy = y - s_win[2 * w], wx = x - s_win[2 * w + 1];
    if (wy < 0 || wy >= S || wx < 0 || wx >= S) continue;
    const float e = load(w, wy * S + wx);
    acc = count ? acc + e : e;
    ++count;
  }
  return acc / (float)count;  // one window: e / 1.0f = e, bit for bit
}

// generic form: one item = one element (row, c, y, x) of the canvas, x fastest - the stores of a wave are contiguous, its
// loads are `ld` floats apart
__global__ void __launch_bounds__(kThreads) k_window_fuse(WindowFuse a) {
  __shared__ int s_win[2 * kMaxWindows];
  load_offsets(a.win, a.n_win, s_win);
  const int SS = a.S * a.S;
  const int64_t plane = (int64_t)a.Hc * a.Wc, n = (int64_t)a.parts * a.Bp * a.C * plane;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % plane);
    const int64_t rc = i / plane;
    const int c = (int)(rc % a.C);
    const int row = (int)(rc / a.C);  // d * Bp + b
    const int d = row / a.Bp, b = row - d * a.Bp;
    const int y = p / a.Wc, x = p - y * a.Wc;
    const float* e = a.e + ((int64_t)d * a.n_win * a.Bp + b) * SS * a.ld + c;
    a.out[i] = fuse_cell(s_win, a.n_win, a.S, y, x,
                         [&](int w, int pix) { return e[((int64_t)w * a.Bp * SS + pix) * a.ld]; });
  }
}

// C = ld = 4 (the latent networks): one item = one canvas pixel, its four channels one 16 B load per covering window - a
// wave's loads are contiguous inside a window's row - and four stores, each contiguous across the wave
__global__ void __launch_bounds__(kThreads) k_window_fuse4(WindowFuse a) {
  __shared__ int s_win[2 * kMaxWindows];
  load_offsets(a.win, a.n_win, s_win);
  const int SS = a.S * a.S;
  const int64_t plane = (int64_t)a.Hc * a.Wc, n = (int64_t)a.parts * a.Bp * plane;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % plane);
    const int row = (int)(i / plane);
    const int d = row / a.Bp, b = row - d * a.Bp;
    const int y = p / a.Wc, x = p - y * a.Wc;
    const float4* e = (const float4*)a.e + ((int64_t)d * a.n_win * a.Bp + b) * SS;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int count = 0;
    for (int w = 0; w < a.n_win; ++w) {
      const int wy = y - s_win[2 * w], wx = x - s_win[2 * w + 1];
      if (wy < 0 || wy >= a.S || wx < 0 || wx >= a.S) continue;
      const float4 v = e[(int64_t)w * a.Bp * SS + wy * a.S + wx];
      if (count) { acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z; acc.w = acc.w + v.w; }
      else acc = v;
      ++count;
    }
    const float cf = (float)count;
    float* o = a.out + (int64_t)row * 4 * plane + p;
    o[0] = acc.x / cf; o[plane] = acc.y / cf; o[2 * plane] = acc.z / cf; o[3 * plane] = acc.w / cf;
  }
}

}  // namespace

void launch_window_gather(hipStream_t st, const WindowGather& a) {
  CD_CHECK(a.n_win >= 1 && a.n_win <= kMaxWindows && a.cpad % 8 == 0 && a.C <= a.cpad && a.Hc >= a.S && a.Wc >= a.S,
           "window gather: bad geometry");
  const int64_t n = (int64_t)a.n_win * a.Bp * a.S * a.S * (a.cpad / 8);
  hipLaunchKernelGGL(k_window_gather, win_grid(n), dim3(kThreads), 0, st, a);
}

void launch_window_fuse(hipStream_t st, const WindowFuse& a) {
  CD_CHECK(a.n_win >= 1 && a.n_win <= kMaxWindows && a.C <= a.ld && a.parts >= 1 && a.Hc >= a.S && a.Wc >= a.S,
           "window fuse: bad geometry");
  const int64_t cells = (int64_t)a.parts * a.Bp * a.Hc * a.Wc;
  if (a.C == 4 && a.ld == 4 && ((uintptr_t)a.e & 15) == 0)
    hipLaunchKernelGGL(k_window_fuse4, win_grid(cells), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL(k_window_fuse, win_grid(cells * a.C), dim3(kThreads), 0, st, a);
}

}  // namespace cd

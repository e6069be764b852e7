// Keep-mask estimation from the two prompts (DiffEdit, Couairon et al. 2022, step 1): the region to edit is where
// the noise predicted under the source prompt and under the target prompt disagree, averaged over a few noised copies of the
// source latent. fp32 throughout, contraction off, every sum in a fixed order, no atomics; a sample reads nothing but its own
// tensors. Four launches around the forwards of a call:
//   k_automask_qsample  x_i = qa*x0 + qb*n_i for the draws of one forward, written as that forward's input (16-bit NHWC with
//                       its duplicate half, or fp32 NCHW for the fp32 networks' own layout pass)
//   k_automask_accum    acc[b, p] += sum_c |e_tgt[i, b, c, p] - e_src[i, b, c, p]|, draws ascending, channels ascending inside a
//                       draw; a thread owns its pixels, so the sum does not depend on how the draws are cut into forwards
//   k_automask_sum      per image and block of kSumPix pixels: sum of map = acc / (n C), four strided pixels per thread ascending,
//                       then a halving tree in LDS; one partial per block
//   k_automask_finish   mean[b] = (partials added in ascending block order) / HW, cl = ratio * mean, v = min(map, cl) / cl,
//                       edit = v > thr, dilated by a (2 d + 1)^2 max through an LDS tile with a halo; keep = 1 - edit
// The per-word attention maps reuse k_automask_qsample and keep their two sums here, in the same arithmetic:
//   k_word_map_accumulate  one included layer of a forward into that forward's per-row sums, nearest replication to the latent grid
//   k_word_map_fold        the draws of a forward into the call's sums, ascending; the scale after the last forward
// and the local blend of the coupled loop turns two such running sums into a keep-mask once per step:
//   k_local_blend_mask     pool, image maximum, threshold and union of a decoder row's source and target map
#include "common.h"
#include "gauss.h"
#include "kernels.h"

namespace cd {

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kSumPix = 4 * kThreads;  // pixels per block of k_automask_sum
constexpr int kTile = 16;              // k_automask_finish: output tile side; the halo adds kAutoMaskMaxDilate on every side
constexpr int kTileMax = kTile + 2 * kAutoMaskMaxDilate;

__global__ void __launch_bounds__(kThreads) k_automask_qsample(AutoMaskNoised a) {
  const int64_t chw = (int64_t)a.C * a.HW, per = (int64_t)a.B * chw, n = (int64_t)a.n_draws * per;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / per);
    const int64_t r = e - (int64_t)i * per;  // the flat index in [B, C, H, W]: the element index of the draw
    const float nz = a.noise ? a.noise[e] : philox_normal(a.seed, a.stream0 + (uint32_t)i, (uint64_t)r);
    const float a0 = a.qa * a.x0[r];
    const float a1 = a.qb * nz;
    const float v = a0 + a1;
    if (a.xq) a.xq[e] = v;
    if (a.xin.xin) {
      const int b = (int)(r / chw);
      const int64_t rem = r - (int64_t)b * chw;
      const int c = (int)(rem / a.HW), p = (int)(rem - (int64_t)c * a.HW);
      const size_t rows = (size_t)a.n_draws * a.B;
      const size_t at = (((size_t)i * a.B + b) * a.HW + p) * a.xin.cpad + c;
      const bf16_t h = f2bf(v + 0.f);  // + 0.f: the layout kernel's x * 1 + 0 (a -0 arrives as +0 there too)
      a.xin.xin[at] = h;
      if (a.xin.dup) a.xin.xin[at + rows * a.HW * a.xin.cpad] = h;
    }
  }
}

// MODE 0: one pixel per thread, scalar loads. 1: one pixel per thread, four channels per 16-byte load (channels contiguous:
// the network's NHWC output). 2: four pixels per thread and 16-byte load (pixels contiguous: NCHW tensors).
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_automask_accum(AutoMaskArgs a) {
  const int HW = a.H * a.W, b = blockIdx.y;
  const int p = (blockIdx.x * kThreads + threadIdx.x) * (MODE == 2 ? 4 : 1);
  if (p >= HW) return;
  float* accp = a.acc + (int64_t)b * HW + p;
  if constexpr (MODE == 2) {
    float4 acc = a.first ? make_float4(0.f, 0.f, 0.f, 0.f) : *(const float4*)accp;
    for (int i = 0; i < a.n_chunk; ++i) {
      const int64_t row = ((int64_t)i * a.B + b) * a.sb + p;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int c = 0; c < a.C; ++c) {
        const float4 et = *(const float4*)(a.e_tgt + row + (int64_t)c * a.sc);
        const float4 es = *(const float4*)(a.e_src + row + (int64_t)c * a.sc);
        s.x += fabsf(et.x - es.x);
        s.y += fabsf(et.y - es.y);
        s.z += fabsf(et.z - es.z);
        s.w += fabsf(et.w - es.w);
      }
      acc.x += s.x; acc.y += s.y; acc.z += s.z; acc.w += s.w;
    }
    *(float4*)accp = acc;
  } else {
    float acc = a.first ? 0.f : *accp;
    for (int i = 0; i < a.n_chunk; ++i) {
      const int64_t row = ((int64_t)i * a.B + b) * a.sb + (int64_t)p * a.sp;
      float s = 0.f;
      if constexpr (MODE == 1) {
        for (int c = 0; c < a.C; c += 4) {
          const float4 et = *(const float4*)(a.e_tgt + row + c);
          const float4 es = *(const float4*)(a.e_src + row + c);
          s += fabsf(et.x - es.x);
          s += fabsf(et.y - es.y);
          s += fabsf(et.z - es.z);
          s += fabsf(et.w - es.w);
        }
      } else {
        for (int c = 0; c < a.C; ++c)
          s += fabsf(a.e_tgt[row + (int64_t)c * a.sc] - a.e_src[row + (int64_t)c * a.sc]);
      }
      acc += s;
    }
    *accp = acc;
  }
}

__device__ inline float map_of(const AutoMaskArgs& a, float acc) { return acc / (float)(a.n_total * a.C); }

__global__ void __launch_bounds__(kThreads) k_automask_sum(AutoMaskArgs a) {
  __shared__ float red[kThreads];
  const int HW = a.H * a.W, b = blockIdx.y, tid = threadIdx.x;
  const float* accb = a.acc + (int64_t)b * HW;
  float s = 0.f;
  for (int j = 0; j < kSumPix / kThreads; ++j) {
    const int p = blockIdx.x * kSumPix + j * kThreads + tid;
    if (p < HW) s += map_of(a, accb[p]);
  }
  red[tid] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] = red[tid] + red[tid + w];
    __syncthreads();
  }
  if (tid == 0) a.partial[(int64_t)b * a.nblk + blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kThreads) k_automask_finish(AutoMaskArgs a) {
  __shared__ float s_cl;
  __shared__ unsigned char edit[kTileMax * kTileMax];
  const int H = a.H, W = a.W, HW = H * W, d = a.dilate, b = blockIdx.z, tid = threadIdx.x;
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile, tw = kTile + 2 * d;
  if (tid == 0) {
    float sum = 0.f;
    for (int k = 0; k < a.nblk; ++k) sum += a.partial[(int64_t)b * a.nblk + k];
    const float mean = sum / (float)HW;
    s_cl = a.ratio * mean;
    if (a.mean_out && blockIdx.x == 0 && blockIdx.y == 0) a.mean_out[b] = mean;
  }
  __syncthreads();
  const float cl = s_cl;
  const float* accb = a.acc + (int64_t)b * HW;
  for (int idx = tid; idx < tw * tw; idx += kThreads) {
    const int ty = idx / tw, tx = idx - ty * tw, y = y0 - d + ty, x = x0 - d + tx;
    unsigned char e = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const float m = map_of(a, accb[y * W + x]);
      const float v = cl == 0.f ? 0.f : fminf(m, cl) / cl;
      e = v > a.thr ? 1 : 0;
    }
    edit[idx] = e;
  }
  __syncthreads();
  const int ly = tid / kTile, lx = tid - ly * kTile, y = y0 + ly, x = x0 + lx;
  if (y >= H || x >= W) return;
  unsigned char e = 0;
  for (int dy = 0; dy <= 2 * d; ++dy)
    for (int dx = 0; dx <= 2 * d; ++dx) e |= edit[(ly + dy) * tw + lx + dx];
  const int64_t at = (int64_t)b * HW + y * W + x;
  a.keep_out[at] = e ? 0.f : 1.f;
  if (a.map_out) a.map_out[at] = map_of(a, accb[y * W + x]);
}

// ---- per-word attention maps: the two sums around cd_word_maps' forwards, grid-stride, a thread owns its elements
__global__ void __launch_bounds__(kThreads) k_word_map_accumulate(WordMapAccum a) {
  const int f = a.h / a.s;
  const int64_t hw = (int64_t)a.h * a.w, n = (int64_t)a.rows * a.N * hw;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t rn = e / hw;  // row * N + word
    const int pix = (int)(e - rn * hw), y = pix / a.w, x = pix - y * a.w;
    const float v = a.layer[rn * a.s * a.s + (y / f) * a.s + x / f];
    a.acc[e] = a.first ? v : a.acc[e] + v;
  }
}

__global__ void __launch_bounds__(kThreads) k_word_map_fold(WordMapFold a) {
  const int64_t n = (int64_t)a.B * a.per;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    float t = a.first ? 0.f : a.total[e];
    for (int i = 0; i < a.n_chunk; ++i) t += a.acc[(int64_t)i * n + e];  // draws ascending
    a.total[e] = t;
    if (a.out) a.out[e] = t * a.scale;
  }
}

// ---- prompt-to-prompt local blend: the keep-mask of one decoder row per workgroup. Both running sums of the
// row are staged in LDS, the (pool x pool) maximum reads them from there, the image maximum is a wave reduction followed by
// one over the waves (max does not depend on the order), and the 0 / 1 cells leave as f x f replicated stores, a row of the
// output per pass of the workgroup. The pool is computed twice - ahead of the maximum and for the compare - rather than kept.
__device__ inline float pooled_max(const float* m, int s, int y, int x, int r) {
  const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > s - 1 ? s - 1 : y + r;
  const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r > s - 1 ? s - 1 : x + r;
  float p = m[y0 * s + x0];
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) p = fmaxf(p, m[yy * s + xx]);
  return p;
}

__global__ void __launch_bounds__(kThreads) k_local_blend_mask(LocalBlendMask a) {
  __shared__ float maps[2][kBlendMaxSide * kBlendMaxSide];
  __shared__ unsigned char edit[kBlendMaxSide * kBlendMaxSide];
  __shared__ float wmax[2][kThreads / 64];
  const int r = blockIdx.x, tid = threadIdx.x, s = a.side, n = s * s, rad = a.pool / 2;
  const float* src = a.acc_src + (int64_t)(r % a.B) * n;
  const float* tgt = a.acc_tgt + (int64_t)r * n;
  for (int i = tid; i < n; i += kThreads) {
    maps[0][i] = src[i];
    maps[1][i] = tgt[i];
  }
  __syncthreads();
  float m0 = 0.f, m1 = 0.f;  // the sums are of softmax mass times weights; a map that is nowhere above 0 edits nowhere
  for (int i = tid; i < n; i += kThreads) {
    const int y = i / s, x = i - y * s;
    m0 = fmaxf(m0, pooled_max(maps[0], s, y, x, rad));
    m1 = fmaxf(m1, pooled_max(maps[1], s, y, x, rad));
  }
  for (int o = 32; o > 0; o >>= 1) {
    m0 = fmaxf(m0, __shfl_xor(m0, o, 64));
    m1 = fmaxf(m1, __shfl_xor(m1, o, 64));
  }
  if ((tid & 63) == 0) { wmax[0][tid >> 6] = m0; wmax[1][tid >> 6] = m1; }
  __syncthreads();
  float mx0 = wmax[0][0], mx1 = wmax[1][0];
  for (int w = 1; w < kThreads / 64; ++w) { mx0 = fmaxf(mx0, wmax[0][w]); mx1 = fmaxf(mx1, wmax[1][w]); }
  for (int i = tid; i < n; i += kThreads) {
    const int y = i / s, x = i - y * s;
    const bool e0 = mx0 > 0.f && pooled_max(maps[0], s, y, x, rad) / mx0 > a.thr;
    const bool e1 = mx1 > 0.f && pooled_max(maps[1], s, y, x, rad) / mx1 > a.thr;
    edit[i] = (e0 || e1) ? 1 : 0;
  }
  __syncthreads();
  const int w = s * a.f, hw = w * w;
  float* keep = a.keep + (int64_t)r * hw;
  for (int o = tid; o < hw; o += kThreads) {
    const int y = o / w, x = o - y * w;
    keep[o] = edit[(y / a.f) * s + x / a.f] ? 0.f : 1.f;
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

void check_automask(const AutoMaskArgs& a) {
  CD_CHECK(a.B > 0 && a.B <= 65535 && a.C > 0 && a.H > 0 && a.W > 0 && (int64_t)a.H * a.W < (1 << 30), "bad keep-mask geometry");
  CD_CHECK(a.dilate >= 0 && a.dilate <= kAutoMaskMaxDilate, "dilate must lie in [0, %d], got %d", kAutoMaskMaxDilate, a.dilate);
}

}  // namespace

int automask_sum_blocks(int HW) { return ceil_div(HW, kSumPix); }

void launch_automask_qsample(hipStream_t st, const AutoMaskNoised& a) {
  const int64_t nb = ((int64_t)a.n_draws * a.B * a.C * a.HW + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_automask_qsample, dim3((unsigned)(nb > 2048 ? 2048 : (nb < 1 ? 1 : nb))), dim3(kThreads), 0, st, a);
}

void launch_automask_accum(hipStream_t st, const AutoMaskArgs& a) {
  check_automask(a);
  const int HW = a.H * a.W;
  const bool ptrs = al16(a.e_src) && al16(a.e_tgt) && al16(a.acc) && a.sb % 4 == 0;
  if (ptrs && a.sp == 1 && HW % 4 == 0 && a.sc % 4 == 0)
    hipLaunchKernelGGL(k_automask_accum<2>, dim3(ceil_div(HW / 4, kThreads), a.B), dim3(kThreads), 0, st, a);
  else if (ptrs && a.sc == 1 && a.C % 4 == 0 && a.sp % 4 == 0)
    hipLaunchKernelGGL(k_automask_accum<1>, dim3(ceil_div(HW, kThreads), a.B), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL(k_automask_accum<0>, dim3(ceil_div(HW, kThreads), a.B), dim3(kThreads), 0, st, a);
}

void launch_automask_finish(hipStream_t st, const AutoMaskArgs& a) {
  check_automask(a);
  CD_CHECK(a.nblk == automask_sum_blocks(a.H * a.W) && a.partial && a.keep_out && a.n_total > 0, "bad keep-mask arguments");
  hipLaunchKernelGGL(k_automask_sum, dim3(a.nblk, a.B), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(k_automask_finish, dim3(ceil_div(a.W, kTile), ceil_div(a.H, kTile), a.B), dim3(kThreads), 0, st, a);
}

void launch_word_map_accumulate(hipStream_t st, const WordMapAccum& a) {
  CD_CHECK(a.layer && a.acc && a.rows > 0 && a.N > 0 && a.s > 0 && a.h > 0 && a.w == a.h, "word maps: empty accumulate");
  CD_CHECK(a.h % a.s == 0, "word maps: a %d x %d token grid does not divide the %d x %d latent", a.s, a.s, a.h, a.w);
  const int64_t nb = ((int64_t)a.rows * a.N * a.h * a.w + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_word_map_accumulate, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(kThreads), 0, st, a);
}

void launch_local_blend_mask(hipStream_t st, const LocalBlendMask& a) {
  CD_CHECK(a.acc_src && a.acc_tgt && a.keep && a.B > 0 && a.Bd > 0 && a.Bd % a.B == 0, "local blend: empty mask launch");
  CD_CHECK(a.side > 0 && a.side <= kBlendMaxSide && a.f > 0 && (int64_t)a.side * a.f <= 32768,
           "local blend: a %d x %d map (at most %d) replicated %d times", a.side, a.side, kBlendMaxSide, a.f);
  CD_CHECK(a.pool >= 1 && a.pool <= kBlendMaxPool && a.pool % 2 == 1, "local blend: pool = %d is not an odd number in [1, %d]",
           a.pool, kBlendMaxPool);
  hipLaunchKernelGGL(k_local_blend_mask, dim3(a.Bd), dim3(kThreads), 0, st, a);
}

void launch_word_map_fold(hipStream_t st, const WordMapFold& a) {
  CD_CHECK(a.acc && a.total && a.n_chunk > 0 && a.B > 0 && a.per > 0, "word maps: empty fold");
  const int64_t nb = ((int64_t)a.B * a.per + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_word_map_fold, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(kThreads), 0, st, a);
}

}  // namespace cd

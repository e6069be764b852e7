// Fused per-step scheduler kernels: DPM-Encoder posterior sample + eps extraction, and the
// coupled DDIM/DDPM decode step with injected eps.
//
// Reference arithmetic being reproduced (same fp32 operation order, contraction off):
//   latent : DDIMSampler.sample_xt_next / compute_eps / p_sample_ddim_with_eps
//            (model/lib/stable_diffusion/ldm/models/diffusion/ddim.py:582-601, 545-580, 603-646)
//   pixel  : sample_xt / sample_xt_next / compute_eps / denoising_step_with_eps
//            (model/gan_wrapper/ddpm_ddim_wrapper.py:310-314, 283-307, 230-280, 114-227)
//            denoising_step (model/lib/ddpm_ddim/utils/diffusion_utils.py:23-136)
//
// All latents / images / z are fp32 NCHW at this level (the reference's layout); one launch per
// sampler step, no host synchronisation: the step's coefficients come from a device-resident
// table indexed by an immediate or by a device-side step counter (hipGraph friendly).
#include "common.h"
#include "kernels.h"

namespace cd {

#pragma clang fp contract(off)

// ---------------- counter-based RNG (Philox4x32-10 + Box-Muller) for throughput runs ----------
__device__ inline void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ inline float philox_normal(uint64_t seed, uint32_t stream, uint64_t idx) {
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
  float rad = sqrtf(-2.0f * __logf(u1));
  float ang = 6.28318530717958647692f * u2;
  return (idx & 1) ? rad * __sinf(ang) : rad * __cosf(ang);
}

__device__ inline const StepCoef& pick(const StepCoef* tab, const int* step_ptr, int step_imm) {
  int s = step_ptr ? *step_ptr : step_imm;
  return tab[s];
}

__device__ inline void write_xin(bf16_t* xin, int xin_cpad, int cfg_dup, int B, int C, int HW,
                                 int b, int c, int p, float v) {
  if (!xin) return;
  bf16_t h = f2bf(v);
  size_t o = ((size_t)b * HW + p) * xin_cpad + c;
  xin[o] = h;
  if (cfg_dup) xin[o + (size_t)B * HW * xin_cpad] = h;
}

// x_T = sqrt(a)*x0 + sqrt(1-a)*n      (ddim.py:477-479; ddpm_ddim_wrapper.py:310-314)
// Also scales the raw input when `pre_scale` is set: x0 = (img - 0.5) * 2 (sd_wrapper:176) is done by caller.
__global__ void k_init_xt(const float* __restrict__ x0, const float* __restrict__ noise,
                          uint64_t seed, uint32_t stream, float* __restrict__ xt,
                          float* __restrict__ z, int64_t z_bstride, int B, int C, int HW,
                          const StepCoef* tab, int step_imm, bf16_t* xin, int xin_cpad,
                          int cfg_dup) {
  int64_t n = (int64_t)B * C * HW;
  const StepCoef co = tab[step_imm];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int b = (int)(i / ((int64_t)C * HW));
    int64_t rem = i - (int64_t)b * C * HW;
    int c = (int)(rem / HW), p = (int)(rem - (int64_t)c * HW);
    float nz = noise ? noise[i] : philox_normal(seed, stream, (uint64_t)i);
    float v = co.sa * x0[i] + co.s1a * nz;
    xt[i] = v;
    if (z) z[(int64_t)b * z_bstride + rem] = v;
    write_xin(xin, xin_cpad, cfg_dup, B, C, HW, b, c, p, v);
  }
}

// combine classifier-free guidance: e = e_u + g*(e_c - e_u)   (ddim.py:555-559)
__device__ inline float load_eps_hat(const float* eh, int64_t sb, int64_t sc, int64_t sp, int b,
                                     int c, int p, int B, int cfg, float g) {
  float e = eh[(int64_t)b * sb + (int64_t)c * sc + (int64_t)p * sp];
  if (cfg) {
    float ec = eh[(int64_t)(b + B) * sb + (int64_t)c * sc + (int64_t)p * sp];
    e = e + g * (ec - e);  // first half of the 2B batch is the unconditional branch
  }
  return e;
}

// One DPM-Encoder step (DDIM-eta form; latent and pixel 'ddim'):
//   x_next = last ? x0 : sap*x0 + dirc*((x_t - sa*x0)/s1a) + sigma*n
//   x0_hat = (x_t - r*e)/sa ;  eps = (x_next - sap*x0_hat - dirc*e)/sigma
//   z[:, slot] = eps ; x_t <- x_next ; next U-Net input <- bf16(x_next)
__global__ void k_encode_step_ddim(const float* __restrict__ x0, float* __restrict__ xt,
                                   const float* __restrict__ eh, int64_t eh_sb, int64_t eh_sc,
                                   int64_t eh_sp, int cfg, float g, const float* __restrict__ gvec,
                                   const float* __restrict__ noise, uint64_t seed,
                                   uint32_t stream, float* __restrict__ z, int64_t z_bstride,
                                   int B, int C, int HW, const StepCoef* tab, const int* step_ptr,
                                   int step_imm, int is_last, bf16_t* xin, int xin_cpad,
                                   int cfg_dup_next) {
  int64_t n = (int64_t)B * C * HW;
  const StepCoef co = pick(tab, step_ptr, step_imm);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int b = (int)(i / ((int64_t)C * HW));
    int64_t rem = i - (int64_t)b * C * HW;
    int c = (int)(rem / HW), p = (int)(rem - (int64_t)c * HW);
    float x0v = x0[i], xtv = xt[i];
    float xn;
    if (is_last) {
      xn = x0v;  // sample_xt_next returns x0 at index 0, no RNG draw (ddim.py:583-584)
    } else {
      float nz = noise ? noise[i] : philox_normal(seed, stream, (uint64_t)i);
      float et = (xtv - co.sa * x0v) / co.s1a;
      float dir = co.dirc * et;
      float nn = co.sigma * nz;
      xn = co.sap * x0v + dir + nn;
    }
    float e = load_eps_hat(eh, eh_sb, eh_sc, eh_sp, b, c, p, B, cfg, gvec ? gvec[b] : g);
    float px0 = (xtv - co.r * e) / co.sa;
    float dir2 = co.dirc * e;
    float eps = (xn - co.sap * px0 - dir2) / co.sigma;
    z[(int64_t)b * z_bstride + rem] = eps;
    xt[i] = xn;
    write_xin(xin, xin_cpad, cfg_dup_next, B, C, HW, b, c, p, xn);
  }
}

// One decode step with injected eps (DDIM-eta form):
//   x0_hat = (x - r*e)/sa ;  x <- sap*x0_hat + dirc*e + sigma*eps      (ddim.py:634-645)
// eps == nullptr -> fresh Gaussian noise (diffusion_utils.denoising_step; refinement loop).
__global__ void k_decode_step_ddim(float* __restrict__ x, const float* __restrict__ eh,
                                   int64_t eh_sb, int64_t eh_sc, int64_t eh_sp, int cfg, float g,
                                   const float* __restrict__ gvec,
                                   const float* __restrict__ eps, int64_t eps_bstride,
                                   const float* __restrict__ noise, uint64_t seed,
                                   uint32_t stream, int B, int C, int HW, const StepCoef* tab,
                                   const int* step_ptr, int step_imm, bf16_t* xin, int xin_cpad,
                                   int cfg_dup_next, float* __restrict__ x0_pred, int eps_bmod) {
  int64_t n = (int64_t)B * C * HW;
  const StepCoef co = pick(tab, step_ptr, step_imm);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int b = (int)(i / ((int64_t)C * HW));
    int64_t rem = i - (int64_t)b * C * HW;
    int c = (int)(rem / HW), p = (int)(rem - (int64_t)c * HW);
    float xv = x[i];
    float e = load_eps_hat(eh, eh_sb, eh_sc, eh_sp, b, c, p, B, cfg, gvec ? gvec[b] : g);
    float px0 = (xv - co.r * e) / co.sa;
    float dir = co.dirc * e;
    // sigma == 0 (eta = 0 tables: DDIB's inversion and decode) reads and draws no noise: the term is +0 either way
    float nn = 0.f;
    if (co.sigma != 0.f) {
      float nz;
      if (eps) nz = eps[(int64_t)(eps_bmod ? b % eps_bmod : b) * eps_bstride + rem];
      else nz = noise ? noise[i] : philox_normal(seed, stream, (uint64_t)i);
      nn = co.sigma * nz;
    }
    float xn = co.sap * px0 + dir + nn;
    x[i] = xn;
    if (x0_pred) x0_pred[i] = px0;
    write_xin(xin, xin_cpad, cfg_dup_next, B, C, HW, b, c, p, xn);
  }
}

// Pixel 'ddpm' posterior form (ddpm_ddim_wrapper.py:291-298, 264-269). Coefficient slots reused:
//   sa=w0, s1a=wt, sap=sqrt(var), dirc=weight(bt/sqrt(1-at)), sigma=exp(0.5*logvar), r=1/sqrt(1-bt)
__global__ void k_encode_step_ddpm(const float* __restrict__ x0, float* __restrict__ xt,
                                   const float* __restrict__ eh, int64_t eh_sb, int64_t eh_sc,
                                   int64_t eh_sp, const float* __restrict__ noise, uint64_t seed,
                                   uint32_t stream, float* __restrict__ z, int64_t z_bstride,
                                   int B, int C, int HW, const StepCoef* tab, const int* step_ptr,
                                   int step_imm, bf16_t* xin, int xin_cpad) {
  int64_t n = (int64_t)B * C * HW;
  const StepCoef co = pick(tab, step_ptr, step_imm);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int b = (int)(i / ((int64_t)C * HW));
    int64_t rem = i - (int64_t)b * C * HW;
    int c = (int)(rem / HW), p = (int)(rem - (int64_t)c * HW);
    float x0v = x0[i], xtv = xt[i];
    float nz = noise ? noise[i] : philox_normal(seed, stream, (uint64_t)i);
    float mean_q = co.sa * x0v + co.s1a * xtv;
    float xn = mean_q + co.sap * nz;
    float e = eh[(int64_t)b * eh_sb + (int64_t)c * eh_sc + (int64_t)p * eh_sp];
    float mean_p = co.r * (xtv - co.dirc * e);
    float eps = (xn - mean_p) / co.sigma;
    z[(int64_t)b * z_bstride + rem] = eps;
    xt[i] = xn;
    write_xin(xin, xin_cpad, 0, B, C, HW, b, c, p, xn);
  }
}

// x <- mean + mask*exp(0.5*logvar)*eps  (ddpm_ddim_wrapper.py:202-210); mask folded into `sigma`
// by the host (sigma slot = 0 when t == 0 is NOT used: the reference multiplies by mask, so we do too).
__global__ void k_decode_step_ddpm(float* __restrict__ x, const float* __restrict__ eh,
                                   int64_t eh_sb, int64_t eh_sc, int64_t eh_sp,
                                   const float* __restrict__ eps, int64_t eps_bstride,
                                   const float* __restrict__ noise, uint64_t seed,
                                   uint32_t stream, int B, int C, int HW, const StepCoef* tab,
                                   const int* step_ptr, int step_imm, bf16_t* xin,
                                   int xin_cpad, int eps_bmod) {
  int64_t n = (int64_t)B * C * HW;
  const StepCoef co = pick(tab, step_ptr, step_imm);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int b = (int)(i / ((int64_t)C * HW));
    int64_t rem = i - (int64_t)b * C * HW;
    int c = (int)(rem / HW), p = (int)(rem - (int64_t)c * HW);
    float xv = x[i];
    float e = eh[(int64_t)b * eh_sb + (int64_t)c * eh_sc + (int64_t)p * eh_sp];
    float mean_p = co.r * (xv - co.dirc * e);
    float nz;
    if (eps) nz = eps[(int64_t)(eps_bmod ? b % eps_bmod : b) * eps_bstride + rem];
    else nz = noise ? noise[i] : philox_normal(seed, stream, (uint64_t)i);
    float xn = mean_p + co.t_mask * co.sigma * nz;
    x[i] = xn;
    write_xin(xin, xin_cpad, 0, B, C, HW, b, c, p, xn);
  }
}

// ---------------- region-keeping decode (DDIMSampler.ddim_sampling_with_eps(mask=, x0=), ddim.py:427-430) ----------------
// Ahead of EVERY forward the reference replaces the running latent: img = q_sample(x0, ts) * mask + (1. - mask) * img. The
// blend ahead of the forward of level k-1 rides in the tail of decode step k (still one launch per sampler step); the one
// ahead of the first forward is k_mask_blend_init. fp32 operation order as written there: src*m, 1-m, (1-m)*x, then the add.
//   qtab != nullptr ("q_sample"): src = qa*x0 + qb*n  (LatentDiffusion.q_sample, ddpm.py:271-274), n from `noise` or Philox
//   qtab == nullptr ("encoder") : src = the DPM-Encoder's own x_t of that level, as it lies in memory
// sample b reads mask row b % mask_bmod and source row b % src_bmod (ensemble members share their sample's mask).
__device__ inline float mask_blend(const MaskBlend& mk, int b, int64_t chw, int HW, int64_t rem, int p, int64_t i, float xv) {
  float m = mk.mask[(int64_t)(b % mk.mask_bmod) * HW + p];
  float sv = mk.src[(int64_t)(b % mk.src_bmod) * chw + rem];
  if (mk.qtab) {
    const float2 q = mk.qtab[mk.qrow];
    float nz = mk.noise ? mk.noise[i] : philox_normal(mk.seed, mk.stream, (uint64_t)i);
    float a0 = q.x * sv;
    float a1 = q.y * nz;
    sv = a0 + a1;
  }
  float keep = sv * m;
  float om = 1.f - m;
  float free_ = om * xv;
  return keep + free_;
}

// x <- blend(x) ahead of the first forward (x = x_T = z[:, 0]); writes the forward's 16-bit input
__global__ void k_mask_blend_init(float* __restrict__ x, MaskBlend mk, int B, int C, int HW, bf16_t* xin, int xin_cpad,
                                  int cfg_dup) {
  const int64_t chw = (int64_t)C * HW, n = (int64_t)B * chw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int b = (int)(i / chw);
    int64_t rem = i - (int64_t)b * chw;
    int c = (int)(rem / HW), p = (int)(rem - (int64_t)c * HW);
    float v = mask_blend(mk, b, chw, HW, rem, p, i, x[i]);
    x[i] = v;
    write_xin(xin, xin_cpad, cfg_dup, B, C, HW, b, c, p, v);
  }
}

// k_decode_step_ddim followed, unless `blend` is 0 (the last step), by the blend of the next level
__global__ void k_decode_step_ddim_masked(float* __restrict__ x, const float* __restrict__ eh,
                                          int64_t eh_sb, int64_t eh_sc, int64_t eh_sp, int cfg, float g,
                                          const float* __restrict__ gvec,
                                          const float* __restrict__ eps, int64_t eps_bstride,
                                          const float* __restrict__ noise, uint64_t seed,
                                          uint32_t stream, int B, int C, int HW, const StepCoef* tab,
                                          const int* step_ptr, int step_imm, bf16_t* xin, int xin_cpad,
                                          int cfg_dup_next, int eps_bmod, MaskBlend mk, int blend) {
  const int64_t chw = (int64_t)C * HW, n = (int64_t)B * chw;
  const StepCoef co = pick(tab, step_ptr, step_imm);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int b = (int)(i / chw);
    int64_t rem = i - (int64_t)b * chw;
    int c = (int)(rem / HW), p = (int)(rem - (int64_t)c * HW);
    float xv = x[i];
    float e = load_eps_hat(eh, eh_sb, eh_sc, eh_sp, b, c, p, B, cfg, gvec ? gvec[b] : g);
    float px0 = (xv - co.r * e) / co.sa;
    float dir = co.dirc * e;
    float nn = 0.f;
    if (co.sigma != 0.f) {
      float nz;
      if (eps) nz = eps[(int64_t)(eps_bmod ? b % eps_bmod : b) * eps_bstride + rem];
      else nz = noise ? noise[i] : philox_normal(seed, stream, (uint64_t)i);
      nn = co.sigma * nz;
    }
    float xn = co.sap * px0 + dir + nn;
    if (blend) xn = mask_blend(mk, b, chw, HW, rem, p, i, xn);
    x[i] = xn;
    write_xin(xin, xin_cpad, cfg_dup_next, B, C, HW, b, c, p, xn);
  }
}

// step counter for graph-replayed loops
__global__ void k_add_int(int* p, int d) { if (threadIdx.x == 0 && blockIdx.x == 0) *p += d; }
__global__ void k_set_int(int* p, int v) { if (threadIdx.x == 0 && blockIdx.x == 0) *p = v; }

static inline int ew_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
}

void launch_init_xt(hipStream_t st, const float* x0, const float* noise, uint64_t seed,
                    uint32_t stream, float* xt, float* z, int64_t z_bstride, int B, int C, int HW,
                    const StepCoef* tab, int step, bf16_t* xin, int xin_cpad, int cfg_dup) {
  int64_t n = (int64_t)B * C * HW;
  hipLaunchKernelGGL(k_init_xt, dim3(ew_grid(n)), dim3(256), 0, st, x0, noise, seed, stream, xt, z,
                     z_bstride, B, C, HW, tab, step, xin, xin_cpad, cfg_dup);
}

void launch_encode_step(hipStream_t st, int kind, const float* x0, float* xt, const EpsHat& eh,
                        const float* noise, uint64_t seed, uint32_t stream, float* z,
                        int64_t z_bstride, int B, int C, int HW, const StepCoef* tab,
                        const int* step_ptr, int step, int is_last, bf16_t* xin, int xin_cpad,
                        int cfg_dup_next) {
  int64_t n = (int64_t)B * C * HW;
  if (kind == SCHED_DDIM) {
    hipLaunchKernelGGL(k_encode_step_ddim, dim3(ew_grid(n)), dim3(256), 0, st, x0, xt, eh.p,
                       eh.sb, eh.sc, eh.sp, eh.cfg, eh.g, eh.gvec, noise, seed, stream, z, z_bstride, B, C,
                       HW, tab, step_ptr, step, is_last, xin, xin_cpad, cfg_dup_next);
  } else {
    hipLaunchKernelGGL(k_encode_step_ddpm, dim3(ew_grid(n)), dim3(256), 0, st, x0, xt, eh.p,
                       eh.sb, eh.sc, eh.sp, noise, seed, stream, z, z_bstride, B, C, HW, tab,
                       step_ptr, step, xin, xin_cpad);
  }
}

void launch_decode_step(hipStream_t st, int kind, float* x, const EpsHat& eh, const float* eps,
                        int64_t eps_bstride, const float* noise, uint64_t seed, uint32_t stream,
                        int B, int C, int HW, const StepCoef* tab, const int* step_ptr, int step,
                        bf16_t* xin, int xin_cpad, int cfg_dup_next, float* x0_pred, int eps_bmod) {
  int64_t n = (int64_t)B * C * HW;
  if (kind == SCHED_DDIM) {
    hipLaunchKernelGGL(k_decode_step_ddim, dim3(ew_grid(n)), dim3(256), 0, st, x, eh.p, eh.sb,
                       eh.sc, eh.sp, eh.cfg, eh.g, eh.gvec, eps, eps_bstride, noise, seed, stream, B, C, HW,
                       tab, step_ptr, step, xin, xin_cpad, cfg_dup_next, x0_pred, eps_bmod);
  } else {
    hipLaunchKernelGGL(k_decode_step_ddpm, dim3(ew_grid(n)), dim3(256), 0, st, x, eh.p, eh.sb,
                       eh.sc, eh.sp, eps, eps_bstride, noise, seed, stream, B, C, HW, tab,
                       step_ptr, step, xin, xin_cpad, eps_bmod);
  }
}

void launch_mask_blend_init(hipStream_t st, float* x, const MaskBlend& mk, int B, int C, int HW, bf16_t* xin, int xin_cpad,
                            int cfg_dup) {
  int64_t n = (int64_t)B * C * HW;
  hipLaunchKernelGGL(k_mask_blend_init, dim3(ew_grid(n)), dim3(256), 0, st, x, mk, B, C, HW, xin, xin_cpad, cfg_dup);
}

void launch_decode_step_masked(hipStream_t st, float* x, const EpsHat& eh, const float* eps, int64_t eps_bstride,
                               const float* noise, uint64_t seed, uint32_t stream, int B, int C, int HW,
                               const StepCoef* tab, const int* step_ptr, int step, bf16_t* xin, int xin_cpad,
                               int cfg_dup_next, int eps_bmod, const MaskBlend& mk, int blend) {
  int64_t n = (int64_t)B * C * HW;
  hipLaunchKernelGGL(k_decode_step_ddim_masked, dim3(ew_grid(n)), dim3(256), 0, st, x, eh.p, eh.sb, eh.sc, eh.sp, eh.cfg,
                     eh.g, eh.gvec, eps, eps_bstride, noise, seed, stream, B, C, HW, tab, step_ptr, step, xin, xin_cpad,
                     cfg_dup_next, eps_bmod, mk, blend);
}

void launch_set_int(hipStream_t st, int* p, int v) {
  hipLaunchKernelGGL(k_set_int, dim3(1), dim3(64), 0, st, p, v);
}
void launch_add_int(hipStream_t st, int* p, int d) {
  hipLaunchKernelGGL(k_add_int, dim3(1), dim3(64), 0, st, p, d);
}

}  // namespace cd

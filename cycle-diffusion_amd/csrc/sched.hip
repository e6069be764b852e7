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
// table indexed by an immediate. Arguments are the structs of kernels.h, passed by value.
#include "common.h"
#include "gauss.h"
#include "kernels.h"
#include "sched_elem.h"

namespace cd {

#pragma clang fp contract(off)

__device__ inline void write_xin(const XinOut& o, const StepGeom& g, const Elem& e, float v) {
  if (!o.xin) return;
  bf16_t h = f2bf(v);
  size_t at = ((size_t)e.b * g.HW + e.p) * o.cpad + e.c;
  o.xin[at] = h;
  for (int j = 1; j <= o.dup; ++j) o.xin[at + (size_t)j * g.B * g.HW * o.cpad] = h;
}

// combine classifier-free guidance: e = e_u + g*(e_c - e_u)   (ddim.py:555-559)
__device__ inline float load_eps_hat(const EpsHat& eh, int B, const Elem& e) {
  float v = eps_hat_at(eh, e.b, e);
  if (eh.cfg) {
    float g = eh.gvec ? eh.gvec[e.b] : eh.g;
    float ec = eps_hat_at(eh, e.b + B, e);
    v = v + g * (ec - v);  // first half of the 2B batch is the unconditional branch
  }
  return v;
}

// the injected eps of the element, or a fresh draw (diffusion_utils.denoising_step; refinement loop)
__device__ inline float eps_or_draw(const StepArgs& a, const Elem& e) {
  if (a.eps.p) return a.eps.p[(int64_t)(a.eps.bmod ? e.b % a.eps.bmod : e.b) * a.eps.bstride + e.rem];
  return draw(a.gauss, e.i);
}

// x_T = sqrt(a)*x0 + sqrt(1-a)*n      (ddim.py:477-479; ddpm_ddim_wrapper.py:310-314)
// x0 = (img - 0.5) * 2 (sd_wrapper:176) is done by the caller.
__global__ void k_init_xt(StepArgs a) {
  const StepCoef co = a.geom.tab[a.geom.step];
  for_each_elem(a.geom, [&](const Elem& e) {
    float nz = draw(a.gauss, e.i);
    float v = co.sa * a.x0[e.i] + co.s1a * nz;
    a.xt[e.i] = v;
    if (a.z.p) a.z.p[(int64_t)e.b * a.z.bstride + e.rem] = v;
    write_xin(a.xin, a.geom, e, v);
  });
}

// One DPM-Encoder step (DDIM-eta form; latent and pixel 'ddim'):
//   x_next = last ? x0 : sap*x0 + dirc*((x_t - sa*x0)/s1a) + sigma*n
//   x0_hat = (x_t - r*e)/sa ;  eps = (x_next - sap*x0_hat - dirc*e)/sigma
//   z[:, slot] = eps ; x_t <- x_next ; next U-Net input <- bf16(x_next)
__global__ void k_encode_step_ddim(StepArgs a) {
  const StepCoef co = a.geom.tab[a.geom.step];
  for_each_elem(a.geom, [&](const Elem& el) {
    float x0v = a.x0[el.i], xtv = a.xt[el.i];
    float xn;
    if (a.is_last) {
      xn = x0v;  // sample_xt_next returns x0 at index 0, no RNG draw (ddim.py:583-584)
    } else {
      float nz = draw(a.gauss, el.i);
      float et = (xtv - co.sa * x0v) / co.s1a;
      float dir = co.dirc * et;
      float nn = co.sigma * nz;
      xn = co.sap * x0v + dir + nn;
    }
    float e = load_eps_hat(a.eh, a.geom.B, el);
    float px0 = (xtv - co.r * e) / co.sa;
    float dir2 = co.dirc * e;
    float eps = (xn - co.sap * px0 - dir2) / co.sigma;
    a.z.p[(int64_t)el.b * a.z.bstride + el.rem] = eps;
    a.xt[el.i] = xn;
    write_xin(a.xin, a.geom, el, xn);
  });
}

// ---------------- region-keeping decode (DDIMSampler.ddim_sampling_with_eps(mask=, x0=), ddim.py:427-430) ----------------
// Ahead of EVERY forward the reference replaces the running latent: img = q_sample(x0, ts) * mask + (1. - mask) * img. The
// blend ahead of the forward of level k-1 rides in the tail of decode step k (still one launch per sampler step); the one
// ahead of the first forward is k_mask_blend_init. fp32 operation order as written there: src*m, 1-m, (1-m)*x, then the add.
//   qtab != nullptr ("q_sample"): src = qa*x0 + qb*n  (LatentDiffusion.q_sample, ddpm.py:271-274), n from mk.gauss
//   qtab == nullptr ("encoder") : src = the DPM-Encoder's own x_t of that level, as it lies in memory
// sample b reads mask row b % mask_bmod and source row b % src_bmod (ensemble members share their sample's mask).
__device__ inline float mask_blend(const MaskBlend& mk, const StepGeom& g, const Elem& e, float xv) {
  float m = mk.mask[(int64_t)(e.b % mk.mask_bmod) * g.HW + e.p];
  float sv = mk.src[(int64_t)(e.b % mk.src_bmod) * ((int64_t)g.C * g.HW) + e.rem];
  if (mk.qtab) {
    const float2 q = mk.qtab[mk.qrow];
    float nz = draw(mk.gauss, e.i);
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
__global__ void k_mask_blend_init(float* x, MaskBlend mk, StepGeom geom, XinOut xin) {
  for_each_elem(geom, [&](const Elem& e) {
    float v = mask_blend(mk, geom, e, x[e.i]);
    x[e.i] = v;
    write_xin(xin, geom, e, v);
  });
}

// what the masked instantiation of the decode step takes beside StepArgs; the unmasked one takes nothing
template <bool MASKED>
struct MaskTail {};
template <>
struct MaskTail<true> {
  MaskBlend mk;
  int blend;  // 0 on the last step: nothing is blended after it
};

// One decode step with injected eps (DDIM-eta form):
//   x0_hat = (x - r*e)/sa ;  x <- sap*x0_hat + dirc*e + sigma*eps      (ddim.py:634-645)
// MASKED: followed, unless `blend` is 0, by the blend of the next level.
template <bool MASKED>
__global__ void k_decode_step_ddim(StepArgs a, MaskTail<MASKED> mt) {
  const StepCoef co = a.geom.tab[a.geom.step];
  for_each_elem(a.geom, [&](const Elem& el) {
    float xv = a.xt[el.i];
    float e = load_eps_hat(a.eh, a.geom.B, el);
    float px0 = (xv - co.r * e) / co.sa;
    float dir = co.dirc * e;
    // sigma == 0 (eta = 0 tables: DDIB's inversion and decode) reads and draws no noise: the term is +0 either way
    float nn = 0.f;
    if (co.sigma != 0.f) {
      float nz = eps_or_draw(a, el);
      nn = co.sigma * nz;
    }
    float xn = co.sap * px0 + dir + nn;
    if constexpr (MASKED) {
      if (mt.blend) xn = mask_blend(mt.mk, a.geom, el, xn);
    }
    a.xt[el.i] = xn;
    write_xin(a.xin, a.geom, el, xn);
  });
}

// Pixel 'ddpm' posterior form (ddpm_ddim_wrapper.py:291-298, 264-269). Coefficient slots reused:
//   sa=w0, s1a=wt, sap=sqrt(var), dirc=weight(bt/sqrt(1-at)), sigma=exp(0.5*logvar), r=1/sqrt(1-bt)
// No classifier-free-guidance combine: the pixel DDPMs are unconditional, and the samplers refuse a guided 'ddpm' call.
__global__ void k_encode_step_ddpm(StepArgs a) {
  const StepCoef co = a.geom.tab[a.geom.step];
  for_each_elem(a.geom, [&](const Elem& el) {
    float x0v = a.x0[el.i], xtv = a.xt[el.i];
    float nz = draw(a.gauss, el.i);
    float mean_q = co.sa * x0v + co.s1a * xtv;
    float xn = mean_q + co.sap * nz;
    float e = eps_hat_at(a.eh, el.b, el);
    float mean_p = co.r * (xtv - co.dirc * e);
    float eps = (xn - mean_p) / co.sigma;
    a.z.p[(int64_t)el.b * a.z.bstride + el.rem] = eps;
    a.xt[el.i] = xn;
    write_xin(a.xin, a.geom, el, xn);
  });
}

// x <- mean + mask*exp(0.5*logvar)*eps  (ddpm_ddim_wrapper.py:202-210); the reference multiplies by its t == 0 mask
// (t_mask) rather than dropping the term, so we do too.
__global__ void k_decode_step_ddpm(StepArgs a) {
  const StepCoef co = a.geom.tab[a.geom.step];
  for_each_elem(a.geom, [&](const Elem& el) {
    float xv = a.xt[el.i];
    float e = eps_hat_at(a.eh, el.b, el);
    float mean_p = co.r * (xv - co.dirc * e);
    float nz = eps_or_draw(a, el);
    float xn = mean_p + co.t_mask * co.sigma * nz;
    a.xt[el.i] = xn;
    write_xin(a.xin, a.geom, el, xn);
  });
}

void launch_init_xt(hipStream_t st, const StepArgs& a) {
  hipLaunchKernelGGL(k_init_xt, ew_grid(a.geom), dim3(256), 0, st, a);
}

void launch_encode_step(hipStream_t st, int kind, const StepArgs& a) {
  if (kind == SCHED_DDIM) {
    hipLaunchKernelGGL(k_encode_step_ddim, ew_grid(a.geom), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_encode_step_ddpm, ew_grid(a.geom), dim3(256), 0, st, a);
  }
}

void launch_decode_step(hipStream_t st, int kind, const StepArgs& a, const MaskBlend* mk, bool blend) {
  if (mk) {
    hipLaunchKernelGGL(k_decode_step_ddim<true>, ew_grid(a.geom), dim3(256), 0, st, a, MaskTail<true>{*mk, blend ? 1 : 0});
  } else if (kind == SCHED_DDIM) {
    hipLaunchKernelGGL(k_decode_step_ddim<false>, ew_grid(a.geom), dim3(256), 0, st, a, MaskTail<false>{});
  } else {
    hipLaunchKernelGGL(k_decode_step_ddpm, ew_grid(a.geom), dim3(256), 0, st, a);
  }
}

void launch_mask_blend_init(hipStream_t st, const StepArgs& a, const MaskBlend& mk) {
  hipLaunchKernelGGL(k_mask_blend_init, ew_grid(a.geom), dim3(256), 0, st, a.xt, mk, a.geom, a.xin);
}

// out[i] = draw(g, first + i): the draws of gauss.h as every kernel above takes them, laid bare for the tests (cd_op_gauss)
__global__ void k_gauss_fill(GaussSrc g, int64_t first, float* out, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    out[i] = draw(g, first + i);
  }
}

void launch_gauss_fill(hipStream_t st, GaussSrc g, int64_t first, float* out, int64_t n) {
  const int64_t nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_gauss_fill, dim3((unsigned)(nb > 2048 ? 2048 : (nb < 1 ? 1 : nb))), dim3(256), 0, st, g, first, out, n);
}

}  // namespace cd

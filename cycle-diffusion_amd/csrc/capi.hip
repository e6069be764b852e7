// extern "C" boundary (include/cyclediff.h): engine lifetime, weight loading, the network forwards and the sampler loops
// (DPM-Encoder / coupled decode). The cd_op_* entry points of the parity tests are in capi_ops.hip.
#include <algorithm>
#include <cmath>

#include "capi_internal.h"

static thread_local std::string g_err;
void set_last_error(const char* what) { g_err = what; }

extern "C" {

const char* cd_last_error(void) { return g_err.c_str(); }
int cd_version(void) { return 101; }
int cd_act_format(void) { return CD_ACT_FP16 ? 1 : 0; }

int cd_engine_create(void* hip_stream, size_t workspace_bytes, cd_handle* out) {
  CD_API_BEGIN
  CD_CHECK(out, "null out pointer");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  CD_CHECK(e == hipSuccess && ndev > 0, "no HIP device available (%s): the engine has no CPU fallback",
           hipGetErrorString(e));
  std::unique_ptr<cd_engine> h(new cd_engine());
  h->st = (hipStream_t)hip_stream;
  if (workspace_bytes < (256u << 20)) workspace_bytes = 256u << 20;
  h->arena.init(workspace_bytes);
  HIP_CHECK(hipMalloc((void**)&h->zeros, 4096));
  HIP_CHECK(hipMemset(h->zeros, 0, 4096));
  {  // implicit-GEMM autotuner (CYCLEDIFF_AUTOTUNE=0 turns it off)
    const char* e = getenv("CYCLEDIFF_AUTOTUNE");
    if (!(e && e[0] == '0') && !g_conv_tuner.scratch) {
      g_conv_tuner.scratch_bytes = (size_t)768 << 20;
      HIP_CHECK(hipMalloc(&g_conv_tuner.scratch, g_conv_tuner.scratch_bytes));
      g_conv_tuner.enabled = true;
    }
  }
  h->splitk.scratch_bytes = (size_t)256 << 20;
  h->splitk.nflags = 1 << 16;
  HIP_CHECK(hipMalloc((void**)&h->splitk.scratch, h->splitk.scratch_bytes));
  HIP_CHECK(hipMalloc((void**)&h->splitk.flags, h->splitk.nflags * sizeof(int)));
  HIP_CHECK(hipMemset(h->splitk.flags, 0, h->splitk.nflags * sizeof(int)));
  HIP_CHECK(hipDeviceSynchronize());
  h->gn_partial_floats = (size_t)1 << 23;  // 32 MB: statistics partials + coefficients of a B = 192 forward (coupled loop, fold 16) need 1.8 M floats
  HIP_CHECK(hipMalloc((void**)&h->gn_partial, h->gn_partial_floats * sizeof(float)));
  h->pacer.init();
  h->coef_staging.init();
  HIP_CHECK(hipHostMalloc((void**)&h->overflow_host, 64, hipHostMallocMapped));
  *h->overflow_host = 0;
  HIP_CHECK(hipHostGetDevicePointer((void**)&h->overflow_dev, h->overflow_host, 0));
  h->op_params_f32.f32 = true; h->op_params_f32.x3 = CD_ACT_FP16 != 0; h->op_params_f32.overflow = h->overflow_dev;
  *out = h.release();
  CD_API_END
}

int cd_engine_destroy(cd_handle h) {
  CD_API_BEGIN
  if (h && h->overflow_host) *h->overflow_host = 0;  // nothing left to report to
  enter_engine(h);
  if (h) {
    (void)hipStreamSynchronize(h->st);
    if (g_conv_prof == h->prof.get()) g_conv_prof = nullptr;
    if (g_conv_splitk.scratch == h->splitk.scratch) g_conv_splitk = SplitKWorkspace();
    if (h->splitk.scratch) (void)hipFree(h->splitk.scratch);
    if (h->splitk.flags) (void)hipFree(h->splitk.flags);
    if (h->zeros) (void)hipFree(h->zeros);
    if (h->gn_partial) (void)hipFree(h->gn_partial);
    h->pacer.destroy();
    h->coef_staging.destroy();
    if (h->overflow_host) (void)hipHostFree(h->overflow_host);
    delete h;
  }
  CD_API_END
}

int cd_engine_synchronize(cd_handle h) {
  CD_API_BEGIN
  CD_CHECK(h, "null handle");
  h->pacer.wait_all(h->st);
  h->check_overflow();
  CD_API_END
}

int cd_prof_enable(cd_handle h, int on) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h, "null handle");
  if (!h->prof) h->prof.reset(new KernelProfiler());
  h->prof->enabled = on != 0;
  {
    const char* e = getenv("CYCLEDIFF_GEMM_LOG");
    h->prof->verbose = e && e[0] == '1';
  }
  g_conv_prof = on ? h->prof.get() : nullptr;
  CD_API_END
}

int cd_prof_collect(cd_handle h, int* launches, double* total_ms, double* total_flops) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && h->prof && launches && total_ms && total_flops, "profiler not enabled");
  HIP_CHECK(hipStreamSynchronize(h->st));
  h->prof->collect(launches, total_ms, total_flops);
  CD_API_END
}

int cd_engine_workspace_high_water(cd_handle h, size_t* bytes) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && bytes, "null argument");
  *bytes = h->arena.high_water();
  CD_API_END
}

int cd_net_create(cd_handle h, const cd_net_desc* d, int* net_id) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && d && net_id, "null argument");
  std::unique_ptr<Net> n;
  switch (d->kind) {
    case CD_NET_UNET_OPENAI: n = make_unet_openai(*d); break;
    case CD_NET_UNET_HO: n = make_unet_ho(*d); break;
    case CD_NET_VAE_KL: n = make_vae_kl(*d); break;
    case CD_NET_CLIP_TEXT:
    case CD_NET_BERT_XTR:
    case CD_NET_OCLIP_TEXT:
    case CD_NET_OCLIP_VISION: n = make_clip_text(*d); break;
    case CD_NET_INCEPTION_FID: n = make_inception_fid(*d); break;
    case CD_NET_LPIPS: n = make_lpips(*d); break;
    default: CD_CHECK(false, "unknown net kind %d", d->kind);
  }
  n->params.overflow = h->overflow_dev;
  h->nets.push_back(std::move(n));
  *net_id = (int)h->nets.size() - 1;
  CD_API_END
}

int cd_net_param_count(cd_handle h, int net, int* n) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && n && net >= 0 && net < (int)h->nets.size(), "bad argument");
  *n = (int)h->nets[net]->params.decls().size();
  CD_API_END
}

int cd_net_param_info(cd_handle h, int net, int index, char* name, int name_cap, int* ndim, int64_t shape[4]) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && net >= 0 && net < (int)h->nets.size(), "bad net id");
  auto& ds = h->nets[net]->params.decls();
  CD_CHECK(index >= 0 && index < (int)ds.size(), "bad parameter index");
  const ParamDecl& d = *ds[index];
  if (name && name_cap > 0) { strncpy(name, d.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (ndim) *ndim = (int)d.shape.size();
  if (shape) for (size_t i = 0; i < 4; ++i) shape[i] = i < d.shape.size() ? d.shape[i] : 1;
  CD_API_END
}

int cd_net_load_param(cd_handle h, int net, const char* name, const float* data_host, int ndim,
                      const int64_t* shape) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && name && data_host && shape && net >= 0 && net < (int)h->nets.size(), "bad argument");
  h->nets[net]->params.load(h->st, name, data_host, ndim, shape);
  CD_API_END
}

int cd_net_missing_params(cd_handle h, int net, int* n_missing, char* first_name, int name_cap) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && n_missing && net >= 0 && net < (int)h->nets.size(), "bad argument");
  std::string first;
  *n_missing = h->nets[net]->params.missing(&first);
  if (first_name && name_cap > 0) { strncpy(first_name, first.c_str(), name_cap - 1); first_name[name_cap - 1] = 0; }
  CD_API_END
}

}  // extern "C"

// ------------------------------------------------------------------ helpers for the forward paths
namespace {

// context rows fp32 [rows][L][Dc] -> rows [row0, row0 + rows) of the context tensor `dst` in the network's format: 16-bit, or -
// fp32 networks (CD_PREC_F32 / F32X3 with transformer blocks) - as they are
void put_ctx(cd_engine* h, const Net* n, const float* src, void* dst, size_t row0, int rows, int L, int Dc) {
  const size_t per = (size_t)L * Dc;
  if (n->f32) HIP_CHECK(hipMemcpyAsync((float*)dst + row0 * per, src, (size_t)rows * per * 4, hipMemcpyDeviceToDevice, h->st));
  else launch_nchw_to_nhwc(h->st, src, (bf16_t*)dst + row0 * per, rows * L, Dc, 1, Dc, 1.f, 0.f, 0);
}

// the context of a forward of B (or, with b, 2 B) rows, optionally [uncond | cond] stacking for classifier-free guidance
bf16_t* make_ctx(cd_engine* h, const Net* n, const float* a, const float* b, int B, int L, int Dc) {
  void* out = h->arena.alloc((size_t)(b ? 2 * B : B) * L * Dc * (n->f32 ? 4 : 2));
  put_ctx(h, n, a, out, 0, B, L, Dc);
  if (b) put_ctx(h, n, b, out, B, B, L, Dc);
  return (bf16_t*)out;
}

// image rows fp32 NCHW [B][C][HW] times `mul` -> the network's input rows [B][HW][cpad]: 16-bit, fp32, or - a split-mode
// network - fp16 pairs; dup: the B samples once more behind themselves (a classifier-free-guidance batch built from one x_t,
// ddim.py:553-559)
void put_net_input(cd_engine* h, const Net* n, const float* src, void* dst, int B, int C, int HW, int cpad, float mul, bool dup) {
  if (!n->f32) { launch_nchw_to_nhwc(h->st, src, (bf16_t*)dst, B, C, HW, cpad, mul, 0.f, dup ? 1 : 0); return; }
  for (int r = 0; r < (dup ? 2 : 1); ++r)
    launch_nchw_to_nhwc_f32(h->st, src, (float*)dst + (size_t)r * B * HW * cpad, B, C, HW, cpad, mul, 0.f, n->x3 ? 1 : 0,
                            h->overflow_dev);
}

struct Guidance {
  bool cfg = false;       // run the 2B batch [uncond | cond]
  const float* ctx_single = nullptr;
};
// ddim.py:550-559: scale==1 -> conditional only; scale==0 -> unconditional only; else CFG
Guidance resolve_guidance(const float* ctx_c, const float* ctx_uc, float g) {
  Guidance r;
  if (!ctx_c && !ctx_uc) return r;
  if (!ctx_uc || g == 1.0f) { r.ctx_single = ctx_c; return r; }
  if (g == 0.0f) { r.ctx_single = ctx_uc; return r; }
  r.cfg = true;
  return r;
}

}  // namespace

// upload_table / upload_coef: capi_ops.hip calls them too (capi_internal.h)
void* upload_table(cd_engine* h, const void* host, size_t bytes) {
  void* d = h->arena.alloc(bytes);
  CoefStaging& cs = h->coef_staging;
  if (cs.host && bytes <= CoefStaging::kSlotBytes) {
    const int slot = cs.next;
    cs.next = (cs.next + 1) % CoefStaging::kSlots;
    StepPacer::sleep_until_done(cs.done[slot]);  // the copy that last used this slot (a never-recorded event is done)
    char* stage = cs.host + (size_t)slot * CoefStaging::kSlotBytes;
    memcpy(stage, host, bytes);
    HIP_CHECK(hipMemcpyAsync(d, stage, bytes, hipMemcpyHostToDevice, h->st));
    HIP_CHECK(hipEventRecord(cs.done[slot], h->st));
  } else {
    HIP_CHECK(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, h->st));
    HIP_CHECK(hipStreamSynchronize(h->st));  // host table may be freed by the caller right after return
  }
  return d;
}

StepCoef* upload_coef(cd_engine* h, const cd_step_coef* host, int n) {
  static_assert(sizeof(cd_step_coef) == sizeof(StepCoef), "coef ABI");
  return (StepCoef*)upload_table(h, host, (size_t)n * sizeof(StepCoef));
}

// the geometry of a set of fused windows, checked on the host before any launch: capi_ops.hip calls it too
void check_window_grid(const int32_t* win_host, int n_win, int Hc, int Wc, int S) {
  const char* fw = "fused windows";
  CD_CHECK(n_win >= 1 && n_win <= kMaxWindows, "%s: n_win = %d outside [0, %d]", fw, n_win, kMaxWindows);
  CD_CHECK(win_host, "%s: win_host is NULL", fw);
  CD_CHECK(S > 0 && Hc >= S && Wc >= S, "%s: a canvas of %d x %d is smaller than the network's %d x %d input", fw, Hc, Wc, S, S);
  CD_CHECK((int64_t)Hc * Wc <= (int64_t)kMaxWindows * S * S, "%s: no window covers every cell of a %d x %d canvas: %d windows "
           "hold fewer cells", fw, Hc, Wc, kMaxWindows);
  std::vector<uint8_t> covered((size_t)Hc * Wc, 0);
  for (int w = 0; w < n_win; ++w) {
    const int y = win_host[2 * w], x = win_host[2 * w + 1];
    CD_CHECK(y >= 0 && x >= 0 && y <= Hc - S && x <= Wc - S, "%s: window %d at (%d, %d) lies outside the %d x %d canvas", fw, w,
             y, x, Hc, Wc);
    for (int v = 0; v < w; ++v)
      CD_CHECK(win_host[2 * v] != y || win_host[2 * v + 1] != x, "%s: windows %d and %d are equal, both at (%d, %d)", fw, v, w,
               y, x);
    for (int yy = y; yy < y + S; ++yy)
      for (int xx = x; xx < x + S; ++xx) covered[(size_t)yy * Wc + xx] = 1;
  }
  for (int i = 0; i < Hc * Wc; ++i)
    CD_CHECK(covered[i], "%s: no window covers canvas cell (%d, %d)", fw, i / Wc, i % Wc);
}

namespace {

// The generator's streams are banded by loop, 4096 streams to a band (tests/_philox_ref.py STREAMS):
// 0 x_T and 1 + i the encoder, 0x1000 + i the decode, 0x2000 / 0x2001 + i the refinement, 0x3000 + j the inversion,
// 0x4000 + slot the keep-mask's q-sample, 0x5000 + i ILVR's reference, 0x6000 + i the keep-mask estimate's draws, 0x7a65 the
// VAE posterior, 0x8000 + i the per-word attention maps' draws. A loop that draws from the
// generator (`noise` is NULL) may not walk into the next loop's numbers; a noise tensor has no such limit.
constexpr int kStreamBandSteps = 0xFFF;
void check_stream_band(const void* noise, int steps, const char* what) {
  CD_CHECK(noise || steps <= kStreamBandSteps,
           "%s = NULL draws from the counter-based generator, whose stream band holds at most %d steps of one loop (got %d): "
           "pass the noise tensor", what, kStreamBandSteps, steps);
}

// the keep-mask of the region-keeping decode and of the coupled loop, checked on the host before any launch; `B` is the
// decoder's batch
void check_mask_args(const cd_keep_mask& m, UNet* u, int sched_kind, int B, bool coupled) {
  CD_CHECK(sched_kind == CD_SCHED_DDIM, "a keep-mask is only defined for sched_kind = CD_SCHED_DDIM (the reference has no mask "
                                        "hook on DDPMDDIMWrapper)");
  CD_CHECK(u->kind() == CD_NET_UNET_OPENAI && u->desc.use_spatial_transformer,
           "a keep-mask is only defined for the latent text networks, not for the pixel networks");
  CD_CHECK(m.mask, "mask is NULL");
  CD_CHECK(m.B_mask > 0 && B % m.B_mask == 0, "mask shape mismatch: %d mask rows for a batch of %d", m.B_mask, B);
  if (m.source == CD_MASK_ENCODER) {
    CD_CHECK(coupled, "mask_source = encoder needs the coupled loop (cd_cycle_translate): the encoder's trajectory "
                      "does not exist in a separate decode");
    CD_CHECK(!m.qsample_coef_host && !m.noise, "mask_source = encoder takes no q-sample table and no mask noise: pass NULL");
  } else {
    CD_CHECK(m.source == CD_MASK_QSAMPLE, "bad mask_source %d", m.source);
    CD_CHECK(m.x0 && m.qsample_coef_host, "mask_source = q_sample needs x0 and the q-sample coefficient table");
  }
}

// the blend of level k (table row k) whose q-sample draw is slot `slot` (the loop's iteration number)
MaskBlend mask_blend_of(const cd_keep_mask& m, const float2* qtab, int k, int slot, int64_t n) {
  MaskBlend b;
  b.mask = m.mask; b.mask_bmod = m.B_mask;
  b.src = m.x0; b.src_bmod = m.B_mask;
  b.qtab = qtab; b.qrow = k;
  b.gauss.noise = m.noise ? m.noise + (int64_t)slot * n : nullptr;
  b.gauss.seed = m.seed; b.gauss.stream = (uint32_t)(0x4000 + slot);
  return b;
}

struct SamplerState {
  UNet* u = nullptr;
  int B = 0, Bn = 0, C = 0, HW = 0, cpad = 0, out_ld = 0;
  bool cfg = false;
  bool f32 = false;  // CD_PREC_F32 network: its NHWC input is fp32 and is rebuilt from xt before every forward
  float g = 1.f;
  float* xt = nullptr;
  bf16_t* xin = nullptr;
  float* eh = nullptr;
  // what the step launches of one call share: xt, the view of eh, B / C / HW, the 16-bit input of the next forward (none for
  // an f32 network). The loops add the table and, per step, the row, the draw and the eps / z pointers.
  StepArgs args;
};

SamplerState setup_sampler(cd_engine* h, int net, const float* ctx_c, const float* ctx_uc, int ctx_len,
                           float guidance, int B) {
  SamplerState s;
  s.u = get_unet(h, net);
  s.B = B; s.C = s.u->desc.in_channels; s.HW = s.u->image_size * s.u->image_size;
  s.cpad = s.u->in_cpad; s.out_ld = s.u->out_channels;
  Guidance gd = resolve_guidance(ctx_c, ctx_uc, guidance);
  s.cfg = gd.cfg; s.g = guidance; s.Bn = s.cfg ? 2 * B : B;
  Ctx c = h->ctx();
  if (ctx_c || ctx_uc) {
    const int Dc = s.u->desc.context_dim;
    CD_CHECK(Dc > 0 && ctx_len > 0, "network has no cross-attention but a context was given");
    bf16_t* cx = s.cfg ? make_ctx(h, s.u, ctx_uc, ctx_c, B, ctx_len, Dc) : make_ctx(h, s.u, gd.ctx_single, nullptr, B, ctx_len, Dc);
    s.u->set_context(c, cx, s.Bn, ctx_len);
  } else {
    CD_CHECK(s.u->desc.context_dim <= 0 || !s.u->desc.use_spatial_transformer,
             "network expects a cross-attention context");
  }
  s.f32 = s.u->f32;
  const size_t esz = s.f32 ? 4 : 2;
  s.xt = (float*)h->arena.alloc((size_t)B * s.C * s.HW * 4);
  s.xin = (bf16_t*)h->arena.alloc((size_t)s.Bn * s.HW * s.cpad * esz);
  HIP_CHECK(hipMemsetAsync(s.xin, 0, (size_t)s.Bn * s.HW * s.cpad * esz, h->st));
  s.eh = (float*)h->arena.alloc((size_t)s.Bn * s.HW * s.out_ld * 4);
  StepArgs& a = s.args;
  a.xt = s.xt;
  a.eh.p = s.eh; a.eh.sb = (int64_t)s.HW * s.out_ld; a.eh.sc = 1; a.eh.sp = s.out_ld;
  a.eh.cfg = s.cfg ? 1 : 0; a.eh.g = guidance;
  a.geom.B = B; a.geom.C = s.C; a.geom.HW = s.HW;
  a.xin.xin = s.f32 ? nullptr : s.xin; a.xin.cpad = s.cpad; a.xin.dup = s.cfg ? 1 : 0;
  return s;
}

void run_unet(cd_engine* h, SamplerState& s, int step) {
  Ctx c = h->ctx();
  if (s.f32) put_net_input(h, s.u, s.xt, s.xin, s.B, s.C, s.HW, s.cpad, 1.f, s.cfg);  // (the 16-bit rows: the step kernels)
  UNetIO io;
  io.xin = s.xin; io.B = s.Bn; io.tab = s.args.geom.tab; io.step = step; io.t_shared = true;
  io.cfg_dup = s.cfg;
  io.out = s.eh; io.out_ld = s.out_ld;
  s.u->forward(c, io);
}

}  // namespace

extern "C" {

int cd_unet_forward(cd_handle h, int net, const float* x, const float* t, const float* ctx, int B,
                    int ctx_len, float* eps_out) {
  CD_API_BEGIN
  enter_engine(h);
  UNet* u = get_unet(h, net);
  CD_CHECK(x && t && eps_out && B > 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  const int C = u->desc.in_channels, HW = u->image_size * u->image_size, Co = u->out_channels;
  if (ctx) {
    const int Dc = u->desc.context_dim;
    CD_CHECK(Dc > 0, "network has no cross-attention");
    bf16_t* cx = make_ctx(h, u, ctx, nullptr, B, ctx_len, Dc);
    u->set_context(c, cx, B, ctx_len);
  }
  bf16_t* xin = (bf16_t*)h->arena.alloc((size_t)B * HW * u->in_cpad * (u->f32 ? 4 : 2));
  put_net_input(h, u, x, xin, B, C, HW, u->in_cpad, 1.f, false);
  float* eh = (float*)h->arena.alloc((size_t)B * HW * Co * 4);
  UNetIO io; io.xin = xin; io.B = B; io.t_explicit = t; io.t_shared = false; io.out = eh; io.out_ld = Co;
  u->forward(c, io);
  launch_nhwc_to_nchw(h->st, eh, 1, Co, eps_out, B, Co, HW, 1.f, 0.f);
  CD_API_END
}

int cd_text_encode(cd_handle h, int net, const int32_t* tokens, int B, int L, float* out) {
  CD_API_BEGIN
  CD_CHECK(h, "null handle");
  enter_engine(h);
  CD_CHECK(net >= 0 && net < (int)h->nets.size() &&
               (h->nets[net]->kind() == CD_NET_CLIP_TEXT || h->nets[net]->kind() == CD_NET_BERT_XTR),
           "net %d is not a text encoder", net);
  CD_CHECK(tokens && out && B > 0 && L > 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  static_cast<TextEncoder*>(h->nets[net].get())->encode(c, (const int*)tokens, B, L, out);
  CD_API_END
}

static TextEncoder* get_tower(cd_handle h, int net, int kind) {
  CD_CHECK(h && net >= 0 && net < (int)h->nets.size() && h->nets[net]->kind() == kind, "net %d has the wrong kind", net);
  return static_cast<TextEncoder*>(h->nets[net].get());
}

int cd_inception_features(cd_handle h, int net, const float* img, int B, int stop_block, float* out) {
  CD_API_BEGIN
  CD_CHECK(h, "null handle");
  enter_engine(h);
  CD_CHECK(net >= 0 && net < (int)h->nets.size(), "bad net id %d", net);
  CD_CHECK(img && out && B > 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  inception_fid_features(h->nets[net].get(), c, img, B, stop_block, out);
  CD_API_END
}

int cd_lpips(cd_handle h, int net, const float* img0, const float* img1, int B, int H, int W, float* per_layer, float* out) {
  CD_API_BEGIN
  CD_CHECK(h, "null handle");
  enter_engine(h);
  CD_CHECK(net >= 0 && net < (int)h->nets.size(), "bad net id %d", net);
  CD_CHECK(img0 && img1 && out, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  lpips_distance(h->nets[net].get(), c, img0, img1, B, H, W, per_layer, out);
  CD_API_END
}

int cd_lpips_tap(cd_handle h, int net, const float* img, int B, int H, int W, int tap, float* out) {
  CD_API_BEGIN
  CD_CHECK(h, "null handle");
  enter_engine(h);
  CD_CHECK(net >= 0 && net < (int)h->nets.size(), "bad net id %d", net);
  CD_CHECK(img && out, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  lpips_tap(h->nets[net].get(), c, img, B, H, W, tap, out);
  CD_API_END
}

int cd_clip_text_features(cd_handle h, int net, const int32_t* tokens, int B, int L, float* out) {
  CD_API_BEGIN
  CD_CHECK(h, "null handle");
  enter_engine(h);
  CD_CHECK(tokens && out && B > 0 && L > 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  get_tower(h, net, CD_NET_OCLIP_TEXT)->text_features(c, (const int*)tokens, B, L, out);
  CD_API_END
}

int cd_clip_image_features(cd_handle h, int net, const float* img, int B, float* out) {
  CD_API_BEGIN
  CD_CHECK(h, "null handle");
  enter_engine(h);
  CD_CHECK(img && out && B > 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  get_tower(h, net, CD_NET_OCLIP_VISION)->image_features(c, img, B, out);
  CD_API_END
}

int cd_vae_encode_hw(cd_handle h, int net, const float* img, const float* noise, uint64_t seed, int B, int H, int W,
                     int sample, float scale, float* z0) {
  CD_API_BEGIN
  enter_engine(h);
  VAE* v = get_vae(h, net);
  CD_CHECK(img && z0 && B > 0 && H > 0 && W > 0, "bad argument");
  CD_CHECK(H % v->factor == 0 && W % v->factor == 0, "first stage: an image of %d x %d is no multiple of the factor %d", H, W,
           v->factor);
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  const int cin = v->desc.in_channels, cp = round_up(cin, 32), hl = H / v->factor, wl = W / v->factor;
  // 16-bit rows, or - first stage in fp32 / in the split mode - fp32 rows / fp16 pairs (the same bytes)
  bf16_t* xin = (bf16_t*)h->arena.alloc((size_t)B * H * W * cp * (v->f32 ? 4 : 2));
  put_net_input(h, v, img, xin, B, cin, H * W, cp, 1.f, false);
  const int mch = v->moments_channels;
  float* mom = (float*)h->arena.alloc((size_t)B * hl * wl * mch * 4);
  v->encode_moments(c, xin, B, H, W, mom);
  // VQ first stage: no distribution, the encoding is the quant_conv output itself (ddpm.py get_first_stage_encoding)
  const bool vq = v->codebook != nullptr;
  launch_posterior_sample(h->st, mom, mch, noise, seed, z0, B, v->desc.embed_dim, hl * wl, scale, (sample && !vq) ? 0 : 1);
  CD_API_END
}

int cd_vae_encode(cd_handle h, int net, const float* img, const float* noise, uint64_t seed, int B, int R,
                  int sample, float scale, float* z0) {
  return cd_vae_encode_hw(h, net, img, noise, seed, B, R, R, sample, scale, z0);
}

int cd_vae_decode_hw(cd_handle h, int net, const float* z0, int B, int hl, int wl, float scale, float out_mul,
                     float out_add, float* img) {
  CD_API_BEGIN
  enter_engine(h);
  VAE* v = get_vae(h, net);
  CD_CHECK(z0 && img && B > 0 && hl > 0 && wl > 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  const int zc = v->desc.embed_dim, cp = round_up(zc, 32), H = hl * v->factor, W = wl * v->factor, co = v->desc.out_channels;
  bf16_t* zin = (bf16_t*)h->arena.alloc((size_t)B * hl * wl * cp * (v->f32 ? 4 : 2));
  if (v->codebook)  // VQModelInterface.decode: quantise to the codebook first (autoencoder.py:274-280)
    launch_vq_quantize(h->st, z0, 1.0f / scale, v->codebook, v->n_embed, zc, B, hl * wl, zin, cp);
  else
    put_net_input(h, v, z0, zin, B, zc, hl * wl, cp, 1.0f / scale, false);  // z = 1/scale * z (ddpm.py:705)
  float* o = (float*)h->arena.alloc((size_t)B * H * W * co * 4);
  v->decode(c, zin, B, hl, wl, o);
  launch_nhwc_to_nchw(h->st, o, 1, co, img, B, co, H * W, out_mul, out_add);
  CD_API_END
}

int cd_vae_decode(cd_handle h, int net, const float* z0, int B, int hlat, float scale, float out_mul,
                  float out_add, float* img) {
  return cd_vae_decode_hw(h, net, z0, B, hlat, hlat, scale, out_mul, out_add, img);
}

int cd_dpm_encode(cd_handle h, int net, int sched_kind, const float* x0, const float* ctx_c,
                  const float* ctx_uc, int ctx_len, float guidance, int B, int K,
                  const cd_step_coef* coef_host, const float* noise, uint64_t seed, int last_uses_x0,
                  float* z_out) {
  CD_API_BEGIN
  enter_engine(h);
  // K = 0: only x_T is drawn (white_box_steps = -1 of the text wrappers: every decode step then draws fresh noise)
  CD_CHECK(h && x0 && coef_host && z_out && B > 0 && K >= 0, "bad argument");
  check_stream_band(noise, K, "cd_dpm_encode: noise");
  ArenaScope arena_scope(h->arena);
  SamplerState s = setup_sampler(h, net, ctx_c, ctx_uc, ctx_len, guidance, B);
  // the 'ddpm' posterior kernels carry no classifier-free-guidance combine (the pixel DDPMs that use them are unconditional,
  // ddpm_ddim_wrapper.py:230-238): a guided call would silently run unguided
  CD_CHECK(sched_kind == CD_SCHED_DDIM || !s.cfg, "classifier-free guidance is only implemented for sched_kind = CD_SCHED_DDIM");
  StepArgs& a = s.args;
  a.geom.tab = upload_coef(h, coef_host, K + 1);
  const int64_t chw = (int64_t)s.C * s.HW, n = (int64_t)B * chw;
  const int64_t zbs = (int64_t)(K + 1) * chw;
  a.x0 = x0; a.gauss.seed = seed; a.z.bstride = zbs;
  a.geom.step = K; a.gauss.noise = noise; a.gauss.stream = 0u; a.z.p = z_out;
  launch_init_xt(h->st, a);
  for (int i = 0; i < K; ++i) {
    const int k = K - 1 - i;
    run_unet(h, s, k);
    const int is_last = (last_uses_x0 && k == 0) ? 1 : 0;
    const float* nz = (noise && !is_last) ? noise + (int64_t)(1 + i) * n : nullptr;
    a.geom.step = k; a.is_last = is_last;
    a.gauss.noise = nz; a.gauss.stream = (uint32_t)(1 + i); a.z.p = z_out + (1 + i) * chw;
    launch_encode_step(h->st, sched_kind, a);
    h->pacer.tick(h->st);
  }
  CD_API_END
}

static void ddim_decode_impl(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps,
                             const float* ctx_c, const float* ctx_uc, int ctx_len, float guidance, const float* gvec,
                             int B, int K, const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed,
                             float* x_out, const cd_keep_mask* mk = nullptr) {
  CD_CHECK(h && z && coef_host && x_out && B > 0 && K > 0 && n_eps <= z_slots - 1, "bad argument");
  check_stream_band(noise_tail, K, "decode: noise_tail");
  if (mk && mk->source == CD_MASK_QSAMPLE) check_stream_band(mk->noise, K, "keep-mask: mask_noise");
  if (mk) check_mask_args(*mk, get_unet(h, net), sched_kind, B, /*coupled=*/false);
  ArenaScope arena_scope(h->arena);
  SamplerState s = setup_sampler(h, net, ctx_c, ctx_uc, ctx_len, guidance, B);
  // the 'ddpm' posterior kernels carry no classifier-free-guidance combine (the pixel DDPMs that use them are unconditional,
  // ddpm_ddim_wrapper.py:230-238): a guided call would silently run unguided
  CD_CHECK(sched_kind == CD_SCHED_DDIM || !s.cfg, "classifier-free guidance is only implemented for sched_kind = CD_SCHED_DDIM");
  if (gvec) {
    CD_CHECK(s.cfg, "per-sample guidance needs the classifier-free-guidance batch (both contexts)");
    s.args.eh.gvec = gvec;
  }
  StepArgs& a = s.args;
  a.geom.tab = upload_coef(h, coef_host, K);
  const int64_t chw = (int64_t)s.C * s.HW, n = (int64_t)B * chw;
  const int64_t zbs = (int64_t)z_slots * chw;
  a.eps.bstride = zbs; a.gauss.seed = seed;
  // x = z[:, 0]  (sd_wrapper:153; ddpm_ddim_wrapper.py:404)
  HIP_CHECK(hipMemcpy2DAsync(s.xt, chw * 4, z, zbs * 4, chw * 4, B, hipMemcpyDeviceToDevice, h->st));
  const float2* qtab = nullptr;
  if (mk) {  // img = q_sample(x0, ts) * mask + (1. - mask) * img ahead of the first forward too (ddim.py:427-430)
    qtab = (const float2*)upload_table(h, mk->qsample_coef_host, (size_t)K * 2 * sizeof(float));
    launch_mask_blend_init(h->st, a, mask_blend_of(*mk, qtab, K - 1, 0, n));
  } else if (!s.f32) launch_nchw_to_nhwc(h->st, s.xt, s.xin, B, s.C, s.HW, s.cpad, 1.f, 0.f, s.cfg ? 1 : 0);
  for (int i = 0; i < K; ++i) {
    const int k = K - 1 - i;
    run_unet(h, s, k);
    const float* eps = (i < n_eps) ? z + (int64_t)(1 + i) * chw : nullptr;
    const float* nz = (!eps && noise_tail) ? noise_tail + (int64_t)(i - n_eps) * n : nullptr;
    a.geom.step = k; a.eps.p = eps;
    a.gauss.noise = nz; a.gauss.stream = (uint32_t)(0x1000 + i);
    if (mk) {
      const MaskBlend next = mask_blend_of(*mk, qtab, k - 1, i + 1, n);
      launch_decode_step(h->st, sched_kind, a, &next, /*blend=*/k > 0);
    } else {
      launch_decode_step(h->st, sched_kind, a);
    }
    h->pacer.tick(h->st);
  }
  HIP_CHECK(hipMemcpyAsync(x_out, s.xt, (size_t)n * 4, hipMemcpyDeviceToDevice, h->st));
}

int cd_ddim_decode(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps,
                   const float* ctx_c, const float* ctx_uc, int ctx_len, float guidance, int B, int K,
                   const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed, float* x_out) {
  CD_API_BEGIN
  enter_engine(h);
  ddim_decode_impl(h, net, sched_kind, z, z_slots, n_eps, ctx_c, ctx_uc, ctx_len, guidance, nullptr, B, K, coef_host,
                   noise_tail, seed, x_out);
  CD_API_END
}

int cd_ddim_decode_v(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps,
                     const float* ctx_c, const float* ctx_uc, int ctx_len, const float* guidance_per_sample, int B,
                     int K, const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed, float* x_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(guidance_per_sample && ctx_c && ctx_uc, "cd_ddim_decode_v: guidance vector and both contexts are required");
  // any scale other than 0 / 1 selects the [uncond | cond] batch (ddim.py:550-559); the vector supplies the values
  ddim_decode_impl(h, net, sched_kind, z, z_slots, n_eps, ctx_c, ctx_uc, ctx_len, 2.0f, guidance_per_sample, B, K,
                   coef_host, noise_tail, seed, x_out);
  CD_API_END
}

// Region-keeping decode: DDIMSampler.sample_with_eps(mask=, x0=) (ddim.py:170-228, 427-430). One launch per sampler step: the
// blend ahead of the forward of level k-1 is the tail of decode step k (sched.hip k_decode_step_ddim<true>).
int cd_ddim_decode_masked(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps, const float* ctx_c,
                          const float* ctx_uc, int ctx_len, float guidance, const float* guidance_per_sample, int B, int K,
                          const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed, const float* mask,
                          const float* x0, int B_mask, int mask_source, const float* qsample_coef_host,
                          const float* mask_noise, uint64_t mask_seed, float* x_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h, "bad argument");
  const cd_keep_mask mk = {mask, x0, B_mask, mask_source, qsample_coef_host, mask_noise, mask_seed};
  if (guidance_per_sample) CD_CHECK(ctx_c && ctx_uc, "cd_ddim_decode_masked: a guidance vector needs both contexts");
  ddim_decode_impl(h, net, sched_kind, z, z_slots, n_eps, ctx_c, ctx_uc, ctx_len, guidance_per_sample ? 2.0f : guidance,
                   guidance_per_sample, B, K, coef_host, noise_tail, seed, x_out, &mk);
  CD_API_END
}

// Deterministic DDIM inversion (DDIB's encoder): DiffusionCLIP's denoising_step(..., eta=0, sampling_type='ddim') walked with
// t_next > t (model/lib/ddpm_ddim/utils/diffusion_utils.py:114-121). With eta = 0 that step is
//   x0_hat = (x - sqrt(1-a_in)*e)/sqrt(a_in) ;  x <- sqrt(a_out)*x0_hat + sqrt(1-a_out)*e
// which is k_decode_step_ddim<false> with sigma = 0 in the same operation order (a sigma = 0 row draws no noise and adds +0), so the
// decode kernel - including its fused write of the next forward's input - runs every step. Rows are in loop order: row j is
// step j, its `t` the timestep of the input's level.
int cd_ddim_invert(cd_handle h, int net, int sched_kind, const float* x0, const float* ctx_c, const float* ctx_uc,
                   int ctx_len, float guidance, int B, int K, const cd_step_coef* coef_host, float* x_out,
                   float* traj_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x0 && coef_host && x_out && B > 0 && K > 0, "bad argument");
  CD_CHECK(sched_kind == CD_SCHED_DDIM, "inversion is only defined for sched_kind = CD_SCHED_DDIM (eta = 0)");
  for (int j = 0; j < K; ++j)
    CD_CHECK(coef_host[j].sigma == 0.f && coef_host[j].sa > 0.f, "inversion row %d: sigma must be 0 and sa > 0", j);
  ArenaScope arena_scope(h->arena);
  SamplerState s = setup_sampler(h, net, ctx_c, ctx_uc, ctx_len, guidance, B);
  StepArgs& a = s.args;
  a.geom.tab = upload_coef(h, coef_host, K);
  const int64_t n = (int64_t)B * s.C * s.HW;
  HIP_CHECK(hipMemcpyAsync(s.xt, x0, (size_t)n * 4, hipMemcpyDeviceToDevice, h->st));
  if (!s.f32) launch_nchw_to_nhwc(h->st, s.xt, s.xin, B, s.C, s.HW, s.cpad, 1.f, 0.f, s.cfg ? 1 : 0);
  for (int j = 0; j < K; ++j) {
    run_unet(h, s, j);
    a.geom.step = j; a.gauss.stream = (uint32_t)(0x3000 + j);
    launch_decode_step(h->st, CD_SCHED_DDIM, a);
    if (traj_out) HIP_CHECK(hipMemcpyAsync(traj_out + (int64_t)j * n, s.xt, (size_t)n * 4, hipMemcpyDeviceToDevice, h->st));
    h->pacer.tick(h->st);
  }
  HIP_CHECK(hipMemcpyAsync(x_out, s.xt, (size_t)n * 4, hipMemcpyDeviceToDevice, h->st));
  CD_API_END
}

// The coupled source -> target loop (north_star): DPM-Encoder step k and decode step k evaluate the SAME network at the SAME
// timestep, and the decode step only needs eps_k AFTER its forward - so both ride in one U-Net batch
//   [ encoder rows (B, or uncond B | cond B under encoder guidance) | decoder rows (Bd = n_dec * B, or uncond Bd | cond Bd) ]
// followed by the encoder's step kernel (x_{k-1}, eps_k -> z) and then the decoder's (consumes eps_k). 99 forwards of
// B + 2 Bd rows instead of 99 of B and 99 of 2 Bd. Per-sample arithmetic is that of cd_dpm_encode followed by cd_ddim_decode(_v).
// The options (include/cyclediff.h: keep-mask, cross-attention control DESIGN.md 14, local blend 18, semantic guidance 20,
// fused windows 21) are branches of this one body; which of them go together is decided here.
// fused windows of cd_cycle_translate (include/cyclediff.h cd_translate_args)
static void check_windows(const cd_translate_args& a, const UNet* u) {
  const char* fw = "fused windows";
  CD_CHECK(a.n_win >= 0 && a.n_win <= kMaxWindows, "%s: n_win = %d outside [0, %d]", fw, a.n_win, kMaxWindows);
  if (a.n_win == 0) {
    CD_CHECK(a.canvas_h == 0 && a.canvas_w == 0 && !a.win_host, "%s: n_win = 0 (off) takes canvas_h = canvas_w = 0 and "
             "win_host = NULL", fw);
    return;
  }
  check_window_grid(a.win_host, a.n_win, a.canvas_h, a.canvas_w, u->image_size);
  CD_CHECK(!u->f32, "%s are not built for precision CD_PREC_F32 / CD_PREC_F32X3 networks: use the 16-bit precision", fw);
  CD_CHECK(!a.mask && !a.ctrl && !a.blend && !a.sega, "%s are not built together with a keep-mask, cross-attention control, the "
           "local blend or concepts yet: call without them", fw);
}

static void cycle_translate_impl(cd_handle h, const cd_translate_args& a) {
  const cd_keep_mask* mk = a.mask;
  const cd_attn_ctrl* ck = a.ctrl;
  const cd_local_blend* bk = a.blend;
  const cd_sega* sk = a.sega;
  CD_CHECK(h && a.x0 && a.coef_enc_host && a.coef_dec_host && a.z_out && a.x_out && a.B > 0 && a.n_dec > 0 && a.K > 0,
           "bad argument");
  CD_CHECK(!(sk && bk), "semantic guidance and the local blend are not built together: call without the blend, or without "
                        "concepts");
  check_stream_band(a.noise, a.K, "cd_cycle_translate: noise");
  if (mk && mk->source == CD_MASK_QSAMPLE) check_stream_band(mk->noise, a.K, "keep-mask: mask_noise");
  ArenaScope arena_scope(h->arena);
  UNet* u = get_unet(h, a.net);
  const int nw = a.n_win;  // fused windows: 0 = off, every launch below is the one of the call without them
  check_windows(a, u);
  const int Bd = a.B * a.n_dec;
  if (mk) check_mask_args(*mk, u, a.sched_kind, a.B, /*coupled=*/true);
  const bool ctrl_on = ck && ck->n_ctrl != 0;
  CD_CHECK(!(mk && bk), "the local blend: a static keep-mask and the local blend exclude each other (the blend "
                        "rewrites the mask after every step)");
  // what the control and the local blend both need of the call; the blend needs it for every n_ctrl
  const bool text_on = ctrl_on || bk;
  const char* what = ctrl_on ? "cross-attention control" : "the local blend";
  if (ck || bk || sk) {
    // one forward serves both passes at the timestep of the DECODER's row k: the two tables must agree on it
    for (int k = 0; k < a.K; ++k)
      CD_CHECK(a.coef_enc_host[k].t == a.coef_dec_host[k].t, "%s: the encoder's and the decoder's tables disagree "
               "on the timestep of row %d (%d against %d)",
               sk ? "semantic guidance" : bk ? "the local blend" : "cross-attention control", k,
               a.coef_enc_host[k].t, a.coef_dec_host[k].t);
  }
  if (sk) {
    const char* sg = "semantic guidance";
    CD_CHECK(sk->E >= 1 && sk->E <= kSegaMaxConcepts, "%s: E = %d concepts outside [1, %d]", sg, sk->E, kSegaMaxConcepts);
    CD_CHECK(sk->edit_ctx && sk->concepts_host, "%s: edit_ctx / concepts_host is NULL", sg);
    CD_CHECK(a.sched_kind == CD_SCHED_DDIM, "%s is only defined for sched_kind = CD_SCHED_DDIM", sg);
    CD_CHECK(u->kind() == CD_NET_UNET_OPENAI && u->desc.use_spatial_transformer && u->desc.context_dim > 0 && a.ctx_len > 0,
             "%s needs a network with a text context: the concepts are contexts", sg);
    CD_CHECK(!u->f32, "%s is not built for precision CD_PREC_F32 / CD_PREC_F32X3 networks: use the 16-bit precision", sg);
    check_sega_params(sk->concepts_host, sk->E, (int64_t)u->desc.in_channels * u->image_size * u->image_size, a.K,
                      sk->momentum_scale, sk->momentum_beta);
  }
  if (text_on) {
    CD_CHECK(a.sched_kind == CD_SCHED_DDIM, "%s is only defined for sched_kind = CD_SCHED_DDIM", what);
    CD_CHECK(u->kind() == CD_NET_UNET_OPENAI && u->desc.use_spatial_transformer && (a.enc_ctx_c || a.enc_ctx_uc),
             "%s needs a network with a text context (and the contexts of both passes)", what);
    CD_CHECK(!u->f32, "%s is not built for fp32 / fp32x3 networks (their transformer blocks run the fp32 "
                      "attention of st_f32.hip): use the 16-bit precision", what);
    CD_CHECK(a.ctx_len <= kCtrlKeys, "%s: context length %d above the %d keys the kernel keeps resident", what, a.ctx_len,
             kCtrlKeys);
  }
  if (bk) {
    const int R = u->image_size;
    CD_CHECK(bk->sel_src && bk->sel_tgt, "the local blend: sel_src / sel_tgt is NULL");
    CD_CHECK(bk->B_sel > 0 && a.B % bk->B_sel == 0, "the local blend shape mismatch: %d selector entries for a batch of %d",
             bk->B_sel, a.B);
    CD_CHECK(bk->side > 0 && bk->side <= kBlendMaxSide, "the local blend: side = %d outside [1, %d] (both maps of a row stay "
             "in LDS)", bk->side, kBlendMaxSide);
    CD_CHECK(R % bk->side == 0, "the local blend: a %d x %d token grid does not divide the %d x %d latent", bk->side, bk->side,
             R, R);
    CD_CHECK(u->count_text_blocks(bk->side, bk->side) > 0, "the local blend: no transformer block has a token grid of side %d",
             bk->side);
    CD_CHECK(bk->pool >= 1 && bk->pool <= kBlendMaxPool && bk->pool % 2 == 1, "the local blend: pool = %d is not an odd number "
             "in [1, %d]", bk->pool, kBlendMaxPool);
    CD_CHECK(bk->n_start >= 0 && bk->n_start <= a.K, "the local blend: n_start = %d outside [0, K = %d]", bk->n_start, a.K);
    CD_CHECK(std::isfinite(bk->thr), "the local blend: the threshold is not finite");
  }
  if (ctrl_on) {
    CD_CHECK(ck->n_ctrl > 0 && ck->n_ctrl <= a.K, "cross-attention control: n_ctrl = %d outside [0, K = %d]", ck->n_ctrl, a.K);
    CD_CHECK(ck->mapper && ck->alpha && ck->weight, "cross-attention control: mapper / alpha / weight is NULL");
    CD_CHECK(ck->B_ctrl > 0 && a.B % ck->B_ctrl == 0, "cross-attention control shape mismatch: %d control rows for a batch "
             "of %d", ck->B_ctrl, a.B);
  }
  // HW: the cells of the running latent - the network's own S x S, or the canvas; HWn: the tokens of one network row; W: the
  // network rows per latent row
  const int C = u->desc.in_channels, HWn = u->image_size * u->image_size, HW = nw ? a.canvas_h * a.canvas_w : HWn;
  const int cpad = u->in_cpad, out_ld = u->out_channels, W = nw ? nw : 1;
  const bool f32 = u->f32;
  Guidance ge = resolve_guidance(a.enc_ctx_c, a.enc_ctx_uc, a.enc_guidance);
  Guidance gd = resolve_guidance(a.dec_ctx_c, a.dec_ctx_uc, a.dec_guidance_per_sample ? 2.0f : a.dec_guidance);
  if (a.dec_guidance_per_sample)
    CD_CHECK(gd.cfg, "per-sample guidance needs the classifier-free-guidance batch (both contexts)");
  if (text_on)
    CD_CHECK((ge.cfg || (a.enc_ctx_c && ge.ctx_single == a.enc_ctx_c)) &&
                 (gd.cfg || (a.dec_ctx_c && gd.ctx_single == a.dec_ctx_c)),
             "%s needs conditional rows in both passes (a guidance scale of 0 runs none)", what);
  CD_CHECK(a.sched_kind == CD_SCHED_DDIM || (!ge.cfg && !gd.cfg), "classifier-free guidance is only implemented for sched_kind = CD_SCHED_DDIM");
  const bool has_ctx = a.enc_ctx_c || a.enc_ctx_uc;
  CD_CHECK(has_ctx == (a.dec_ctx_c || a.dec_ctx_uc), "cd_cycle_translate: contexts for both passes or for neither");
  if (sk)
    CD_CHECK(gd.cfg, "semantic guidance: dec_guidance = %g (or a missing context) leaves the decoder pass without its "
                     "unconditional or its conditional rows; the concept directions are taken against the unconditional row",
             (double)a.dec_guidance);
  // decoder batch rows under semantic guidance: [uncond Bd | concept 0 Bd | ... | concept E-1 Bd | cond Bd]
  const int E = sk ? sk->E : 0;
  const int Ben = ge.cfg ? 2 * a.B : a.B, Bdn = gd.cfg ? (2 + E) * Bd : Bd, Bn = Ben + Bdn;
  Ctx c = h->ctx();
  if (has_ctx) {
    const int Dc = u->desc.context_dim;
    CD_CHECK(Dc > 0 && a.ctx_len > 0, "network has no cross-attention but a context was given");
    // one context tensor in batch-row order: [enc (uncond | cond) | dec (uncond | cond)]
    // (with windows every part is window-major: the part's contexts once per window, in row order)
    void* cx = h->arena.alloc((size_t)Bn * W * a.ctx_len * Dc * (f32 ? 4 : 2));
    auto put = [&](const float* src, int rows, size_t row0) {
      for (int w = 0; w < W; ++w) put_ctx(h, u, src, cx, row0 * W + (size_t)w * rows, rows, a.ctx_len, Dc);
    };
    if (ge.cfg) { put(a.enc_ctx_uc, a.B, 0); put(a.enc_ctx_c, a.B, a.B); } else put(ge.ctx_single, a.B, 0);
    if (gd.cfg) {
      put(a.dec_ctx_uc, Bd, Ben);
      if (sk) put(sk->edit_ctx, E * Bd, Ben + Bd);  // concept-major, as the rows lie
      put(a.dec_ctx_c, Bd, Ben + (size_t)(1 + E) * Bd);
    } else put(gd.ctx_single, Bd, Ben);
    u->set_context(c, (const bf16_t*)cx, Bn * W, a.ctx_len);
  } else {
    CD_CHECK(u->desc.context_dim <= 0 || !u->desc.use_spatial_transformer, "network expects a cross-attention context");
  }
  // the controlled rows are the decoder's conditional rows - the tail of the batch in either layout - and their source the
  // encoder's conditional row of the same sample: V_a / V_b of every block once per call, next to the cached keys and values
  AttnCtrl actl;
  if (ctrl_on) {
    actl.row0 = Bn - Bd; actl.rows = Bd;
    actl.src_b0 = ge.cfg ? a.B : 0; actl.B_src = a.B;
    u->build_attn_control(c, ck->mapper, ck->alpha, ck->weight, ck->B_ctrl, actl);
  }
  const size_t esz = f32 ? 4 : 2;
  const int64_t chw = (int64_t)C * HW, n = (int64_t)a.B * chw;
  // the local blend: the running sums of the encoder's and of the decoder's conditional rows [B | Bd][side][side], collected
  // beside every forward, and the keep-mask [Bd][HW] that k_local_blend_mask rewrites from them once per step
  WordMapCollect wm;
  float *acc = nullptr, *keep = nullptr;
  if (bk) {
    const int ss = bk->side * bk->side;
    acc = (float*)h->arena.alloc((size_t)(a.B + Bd) * ss * 4);
    keep = (float*)h->arena.alloc((size_t)Bd * HW * 4);
    HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)(a.B + Bd) * ss * 4, h->st));
    launch_fill_f32(h->st, keep, 1.f, (int64_t)Bd * HW);
    wm.N = 1; wm.min_side = wm.max_side = bk->side;
    WordMapCollect::Range rs, rt;
    rs.row0 = ge.cfg ? a.B : 0; rs.rows = a.B; rs.sel = bk->sel_src; rs.B_sel = bk->B_sel; rs.acc = acc;
    rt.row0 = Bn - Bd; rt.rows = Bd; rt.sel = bk->sel_tgt; rt.B_sel = bk->B_sel; rt.acc = acc + (size_t)a.B * ss;
    wm.ranges = {rs, rt};
  }
  float* xt_e = (float*)h->arena.alloc((size_t)a.B * chw * 4);
  float* xt_d = (float*)h->arena.alloc((size_t)Bd * chw * 4);
  char* xin = (char*)h->arena.alloc((size_t)Bn * W * HWn * cpad * esz);
  HIP_CHECK(hipMemsetAsync(xin, 0, (size_t)Bn * W * HWn * cpad * esz, h->st));
  float* eh = (float*)h->arena.alloc((size_t)Bn * W * HWn * out_ld * 4);
  const size_t row_in = (size_t)HWn * cpad * esz;  // bytes of one sample of the network input
  bf16_t* xin_e = f32 ? nullptr : (bf16_t*)xin;
  bf16_t* xin_d = f32 ? nullptr : (bf16_t*)(xin + (size_t)Ben * W * row_in);
  StepArgs enc, dec;  // the step launches of the encoder's and of the decoder's rows
  EpsHat &eh_e = enc.eh, &eh_d = dec.eh;
  eh_e.p = eh; eh_e.sb = (int64_t)HWn * out_ld; eh_e.sc = 1; eh_e.sp = out_ld; eh_e.cfg = ge.cfg ? 1 : 0; eh_e.g = a.enc_guidance;
  eh_d = eh_e; eh_d.p = eh + (int64_t)Ben * HWn * out_ld; eh_d.cfg = gd.cfg ? 1 : 0; eh_d.g = a.dec_guidance;
  eh_d.gvec = a.dec_guidance_per_sample;
  // fused windows: the step kernels read the fused eps of the canvas, fp32 NCHW with the [uncond | cond] halves intact (the
  // combine stays theirs), and write no network input - the gathers ahead of every forward do
  WindowGather wg_e, wg_d;
  WindowFuse wf_e, wf_d;
  if (nw) {
    const int* win = (const int*)upload_table(h, a.win_host, (size_t)nw * 2 * sizeof(int32_t));
    float* ehc_e = (float*)h->arena.alloc((size_t)Ben * C * HW * 4);
    float* ehc_d = (float*)h->arena.alloc((size_t)Bdn * C * HW * 4);
    wg_e.x = xt_e; wg_e.y = xin_e; wg_e.win = win; wg_e.Bp = a.B; wg_e.C = C; wg_e.Hc = a.canvas_h; wg_e.Wc = a.canvas_w;
    wg_e.S = u->image_size; wg_e.n_win = nw; wg_e.cpad = cpad; wg_e.dup = ge.cfg ? 1 : 0;
    wg_d = wg_e; wg_d.x = xt_d; wg_d.y = xin_d; wg_d.Bp = Bd; wg_d.dup = gd.cfg ? 1 : 0;
    wf_e.e = eh; wf_e.out = ehc_e; wf_e.win = win; wf_e.Bp = a.B; wf_e.C = C; wf_e.Hc = a.canvas_h; wf_e.Wc = a.canvas_w;
    wf_e.S = u->image_size; wf_e.n_win = nw; wf_e.ld = out_ld; wf_e.parts = ge.cfg ? 2 : 1;
    wf_d = wf_e; wf_d.e = eh + (int64_t)Ben * W * HWn * out_ld; wf_d.out = ehc_d; wf_d.Bp = Bd; wf_d.parts = gd.cfg ? 2 : 1;
    eh_e.p = ehc_e; eh_e.sb = (int64_t)C * HW; eh_e.sc = HW; eh_e.sp = 1;
    eh_d.p = ehc_d; eh_d.sb = (int64_t)C * HW; eh_d.sc = HW; eh_d.sp = 1;
    xin_e = xin_d = nullptr;  // what the step kernels see
  }
  StepCoef* tab_e = upload_coef(h, a.coef_enc_host, a.K + 1);
  StepCoef* tab_d = upload_coef(h, a.coef_dec_host, a.K);
  const int64_t zbs = (int64_t)(a.K + 1) * chw;
  enc.x0 = a.x0; enc.xt = xt_e;
  enc.geom.B = a.B; enc.geom.C = C; enc.geom.HW = HW; enc.geom.tab = tab_e;
  enc.xin.xin = xin_e; enc.xin.cpad = cpad; enc.xin.dup = ge.cfg ? 1 : 0;
  enc.gauss.seed = a.seed; enc.z.bstride = zbs;
  dec.xt = xt_d;
  dec.geom.B = Bd; dec.geom.C = C; dec.geom.HW = HW; dec.geom.tab = tab_d;
  dec.xin.xin = xin_d; dec.xin.cpad = cpad; dec.xin.dup = gd.cfg ? 1 + E : 0;  // every concept row's input is the row's latent
  dec.gauss.seed = a.seed; dec.eps.bstride = zbs; dec.eps.bmod = a.n_dec > 1 ? a.B : 0;
  // semantic guidance: two launches between the forward and the decode step turn u, c and the concept rows into the eps the
  // step reads - fp32 NCHW, no combine left to do (cfg = 0); no step kernel's arithmetic changes
  SegaStep sg;
  if (sk) {
    sg.eh = eh_d;
    sg.Bd = Bd; sg.C = C; sg.HW = HW; sg.E = E;
    sg.tab = (const SegaConcept*)upload_table(h, sk->concepts_host, (size_t)E * sizeof(SegaConcept));
    sg.abuf = (float*)h->arena.alloc((size_t)Bd * E * chw * 4);
    sg.tau = (float*)h->arena.alloc((size_t)a.K * Bd * E * 4);  // [K, Bd, E]: 0 where the concept is inactive
    sg.kept = (int*)h->arena.alloc((size_t)a.K * Bd * E * 4);
    sg.nu = (float*)h->arena.alloc((size_t)Bd * chw * 4);     // zero before iteration 0, nothing kept between calls
    sg.eps = (float*)h->arena.alloc((size_t)Bd * chw * 4);
    sg.s_m = sk->momentum_scale; sg.beta = sk->momentum_beta;
    HIP_CHECK(hipMemsetAsync(sg.tau, 0, (size_t)a.K * Bd * E * 4, h->st));
    HIP_CHECK(hipMemsetAsync(sg.kept, 0, (size_t)a.K * Bd * E * 4, h->st));
    HIP_CHECK(hipMemsetAsync(sg.nu, 0, (size_t)Bd * chw * 4, h->st));
    if (sk->mask_out) HIP_CHECK(hipMemsetAsync(sk->mask_out, 0, (size_t)Bd * E * chw * 4, h->st));
    eh_d.p = sg.eps; eh_d.sb = chw; eh_d.sc = HW; eh_d.sp = 1; eh_d.cfg = 0; eh_d.gvec = nullptr;
  }
  // x_T (ddim.py:477-479), z[:, 0]; the decoder starts from the same tensor (sd_wrapper:153), once per decoder scale
  enc.geom.step = a.K; enc.gauss.noise = a.noise; enc.gauss.stream = 0u; enc.z.p = a.z_out;
  launch_init_xt(h->st, enc);
  for (int j = 0; j < a.n_dec; ++j)
    HIP_CHECK(hipMemcpyAsync(xt_d + (int64_t)j * n, xt_e, (size_t)n * 4, hipMemcpyDeviceToDevice, h->st));
  // the keep-mask blend of level k for the decoder rows: q_sample(x0) with the draw of iteration `slot`, or - "encoder" - the
  // DPM-Encoder's own x_t of that level, which is what xt_e holds once the encoder's step kernel of the iteration has run
  const float2* qtab = nullptr;
  if (mk && mk->source == CD_MASK_QSAMPLE)
    qtab = (const float2*)upload_table(h, mk->qsample_coef_host, (size_t)a.K * 2 * sizeof(float));
  auto blend_of = [&](int k, int slot) {
    MaskBlend b = mask_blend_of(*mk, qtab, k, slot, (int64_t)Bd * chw);
    if (mk->source == CD_MASK_ENCODER) { b.src = xt_e; b.src_bmod = a.B; }
    return b;
  };
  if (mk) launch_mask_blend_init(h->st, dec, blend_of(a.K - 1, 0));
  else if (!f32 && !nw) launch_nchw_to_nhwc(h->st, xt_d, xin_d, Bd, C, HW, cpad, 1.f, 0.f, gd.cfg ? 1 + E : 0);
  // rows that repeat the rows just ahead of them (the decoder's cond half repeats its uncond half): the network computes
  // everything ahead of the first cross-attention once for them - only when the encoder half has no such pair of its own
  // (not under semantic guidance: the shared prefix covers one pair of halves, not the concept rows between them)
  const int dup_tail = (gd.cfg && !ge.cfg && !sk) ? Bd * W : 0;
  for (int i = 0; i < a.K; ++i) {
    const int k = a.K - 1 - i;
    if (f32) {
      put_net_input(h, u, xt_e, xin, a.B, C, HW, cpad, 1.f, ge.cfg);
      put_net_input(h, u, xt_d, xin + (size_t)Ben * row_in, Bd, C, HW, cpad, 1.f, gd.cfg);
    }
    if (nw) { launch_window_gather(h->st, wg_e); launch_window_gather(h->st, wg_d); }
    UNetIO io;
    io.xin = (const bf16_t*)xin; io.B = Bn * W; io.tab = tab_d; io.step = k; io.t_shared = true;  // rows k of both tables carry the same t
    io.dup_tail = dup_tail;
    io.ctrl = (ctrl_on && i < ck->n_ctrl) ? &actl : nullptr;
    io.maps = bk ? &wm : nullptr;
    io.out = eh; io.out_ld = out_ld;
    u->forward(c, io);
    if (nw) { launch_window_fuse(h->st, wf_e); launch_window_fuse(h->st, wf_d); }
    const int is_last = (a.last_uses_x0 && k == 0) ? 1 : 0;
    const float* nz = (a.noise && !is_last) ? a.noise + (int64_t)(1 + i) * n : nullptr;
    float* zslot = a.z_out + (1 + i) * chw;
    enc.geom.step = k; enc.is_last = is_last;
    enc.gauss.noise = nz; enc.gauss.stream = (uint32_t)(1 + i); enc.z.p = zslot;
    launch_encode_step(h->st, a.sched_kind, enc);
    dec.geom.step = k; dec.eps.p = zslot; dec.gauss.stream = (uint32_t)(0x1000 + i);
    if (sk) {
      SegaStep it = sg;
      it.active = sega_active_mask(sk->concepts_host, E, i);
      it.tau = sg.tau + (size_t)i * Bd * E; it.kept = sg.kept + (size_t)i * Bd * E;
      it.mask_out = it.active ? sk->mask_out : nullptr;  // the mask of the last iteration in which a concept was active
      launch_sega_guidance(h->st, it);
    }
    if (mk) {
      const MaskBlend next = blend_of(k - 1, i + 1);
      launch_decode_step(h->st, a.sched_kind, dec, &next, /*blend=*/k > 0);
    } else if (bk && i >= bk->n_start) {
      // the mask of this step from the sums so far, then the step and - the last step included - the blend with the
      // encoder's x of the level just arrived at (xt_e after the encoder's step kernel above)
      LocalBlendMask lm;
      lm.acc_src = acc; lm.acc_tgt = acc + (size_t)a.B * bk->side * bk->side; lm.keep = keep;
      lm.B = a.B; lm.Bd = Bd; lm.side = bk->side; lm.f = u->image_size / bk->side; lm.pool = bk->pool; lm.thr = bk->thr;
      launch_local_blend_mask(h->st, lm);
      MaskBlend lb;
      lb.mask = keep; lb.mask_bmod = Bd; lb.src = xt_e; lb.src_bmod = a.B;
      launch_decode_step(h->st, a.sched_kind, dec, &lb, /*blend=*/true);
    } else {
      launch_decode_step(h->st, a.sched_kind, dec);
    }
    h->pacer.tick(h->st);
  }
  HIP_CHECK(hipMemcpyAsync(a.x_out, xt_d, (size_t)Bd * chw * 4, hipMemcpyDeviceToDevice, h->st));
  if (sk && sk->tau_out)
    HIP_CHECK(hipMemcpyAsync(sk->tau_out, sg.tau, (size_t)a.K * Bd * E * 4, hipMemcpyDeviceToDevice, h->st));
  if (sk && sk->kept_out)
    HIP_CHECK(hipMemcpyAsync(sk->kept_out, sg.kept, (size_t)a.K * Bd * E * 4, hipMemcpyDeviceToDevice, h->st));
  if (bk && bk->acc_out)
    HIP_CHECK(hipMemcpyAsync(bk->acc_out, acc, (size_t)(a.B + Bd) * bk->side * bk->side * 4, hipMemcpyDeviceToDevice, h->st));
  if (bk && bk->keep_out)
    HIP_CHECK(hipMemcpyAsync(bk->keep_out, keep, (size_t)Bd * HW * 4, hipMemcpyDeviceToDevice, h->st));
}

int cd_cycle_translate(cd_handle h, const cd_translate_args* a) {
  CD_API_BEGIN
  CD_CHECK(a, "cd_cycle_translate: the argument struct is NULL");
  CD_CHECK(a->size == sizeof(cd_translate_args), "cd_cycle_translate: the argument struct says size = %u, this library's "
           "sizeof(cd_translate_args) is %zu: built against another version of cyclediff.h?", (unsigned)a->size,
           sizeof(cd_translate_args));
  enter_engine(h);
  cycle_translate_impl(h, *a);
  CD_API_END
}

int cd_pix_refine(cd_handle h, int net, int sched_kind, float* x, int B, int R, const cd_step_coef* coef_host,
                  const float* noise, uint64_t seed) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && coef_host && B > 0 && R > 0, "bad argument");
  check_stream_band(noise, R, "cd_pix_refine: noise");
  ArenaScope arena_scope(h->arena);
  SamplerState s = setup_sampler(h, net, nullptr, nullptr, 0, 1.f, B);
  StepArgs& a = s.args;
  a.geom.tab = upload_coef(h, coef_host, R + 1);
  const int64_t n = (int64_t)B * s.C * s.HW;
  a.x0 = x; a.gauss.seed = seed;
  a.geom.step = R; a.gauss.noise = noise; a.gauss.stream = 0x2000u;
  launch_init_xt(h->st, a);
  for (int i = 0; i < R; ++i) {
    const int k = R - 1 - i;
    run_unet(h, s, k);
    const float* nz = noise ? noise + (int64_t)(1 + i) * n : nullptr;
    a.geom.step = k; a.gauss.noise = nz; a.gauss.stream = (uint32_t)(0x2001 + i);
    launch_decode_step(h->st, sched_kind, a);
    h->pacer.tick(h->st);
  }
  HIP_CHECK(hipMemcpyAsync(x, s.xt, (size_t)n * 4, hipMemcpyDeviceToDevice, h->st));
  CD_API_END
}

}  // extern "C"

// ---- ILVR (csrc/ilvr.hip); cd_op_lowpass in capi_ops.hip shares the two helpers (capi_internal.h)
LowpassTaps upload_taps(cd_engine* h, int n_in, int n_out) {
  std::vector<float> w;
  std::vector<int> first;
  LowpassTaps t;
  t.n_in = n_in; t.n_out = n_out;
  build_lowpass_taps(n_in, n_out, w, first, t.P);
  t.w = (const float*)upload_table(h, w.data(), w.size() * sizeof(float));
  t.first = (const int*)upload_table(h, first.data(), first.size() * sizeof(int));
  return t;
}

void check_lowpass_geometry(int R, int down_n) {
  CD_CHECK(down_n >= 1, "ILVR: down_n must be >= 1, got %d", down_n);
  CD_CHECK(R % down_n == 0, "ILVR: down_n = %d does not divide the resolution %d", down_n, R);
  CD_CHECK(R / down_n >= 4, "ILVR: R / down_n = %d / %d leaves fewer than 4 pixels (the cubic window then reflects twice)", R, down_n);
}

extern "C" {

// ILVR: cd_ddim_decode's loop without contexts; after the decode step of row k > range_t the running image is pulled to
// the reference's low-pass band, x <- x' + phi_N((qa_k y + qb_k n_k) - x'). Rows k <= range_t run the decode step alone.
int cd_ilvr_decode(cd_handle h, int net, int sched_kind, const float* z, int z_slots, int n_eps, int B, int K,
                   const cd_step_coef* coef_host, const float* noise_tail, uint64_t seed, const float* ref, int B_ref,
                   int down_n, int range_t, const float* qsample_coef_host, const float* ref_noise, uint64_t ref_seed,
                   float* x_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && z && coef_host && x_out && ref && B > 0 && K > 0 && n_eps <= z_slots - 1, "bad argument");
  check_stream_band(noise_tail, K, "cd_ilvr_decode: noise_tail");
  check_stream_band(ref_noise, K, "cd_ilvr_decode: ref_noise");
  UNet* u = get_unet(h, net);
  CD_CHECK(!(u->desc.use_spatial_transformer && u->desc.context_dim > 0),
           "ILVR runs on an unconditional pixel DDPM: this network takes a text context");
  const int R = u->image_size;
  check_lowpass_geometry(R, down_n);
  CD_CHECK(range_t >= 0, "ILVR: range_t must be >= 0, got %d", range_t);
  CD_CHECK(B_ref > 0 && B % B_ref == 0, "ILVR: %d reference images for a batch of %d", B_ref, B);
  CD_CHECK(qsample_coef_host, "ILVR: the q-sample coefficient table is NULL");
  ArenaScope arena_scope(h->arena);
  SamplerState s = setup_sampler(h, net, nullptr, nullptr, 0, 1.f, B);
  StepArgs& a = s.args;
  a.geom.tab = upload_coef(h, coef_host, K);
  const int64_t chw = (int64_t)s.C * s.HW, n = (int64_t)B * chw;
  const int64_t zbs = (int64_t)z_slots * chw;
  a.eps.bstride = zbs; a.gauss.seed = seed;
  IlvrArgs iv;
  if (range_t < K - 1) {  // some row is conditioned
    const int r = R / down_n;
    iv.xp = iv.out = s.xt;
    iv.y = ref; iv.y_bmod = B_ref;
    iv.qtab = (const float2*)upload_table(h, qsample_coef_host, (size_t)K * 2 * sizeof(float));
    iv.gauss.seed = ref_seed;
    iv.B = B; iv.C = s.C; iv.R = R;
    iv.D = upload_taps(h, R, r);
    iv.U = upload_taps(h, r, R);
    iv.T = (float*)h->arena.alloc((size_t)B * s.C * r * r * sizeof(float));
    iv.xin = a.xin;
    iv.vec4 = (R % 4 == 0 && aligned16(ref) && aligned16(ref_noise)) ? 1 : 0;
  }
  HIP_CHECK(hipMemcpy2DAsync(s.xt, chw * 4, z, zbs * 4, chw * 4, B, hipMemcpyDeviceToDevice, h->st));
  if (!s.f32) launch_nchw_to_nhwc(h->st, s.xt, s.xin, B, s.C, s.HW, s.cpad, 1.f, 0.f, 0);
  for (int i = 0; i < K; ++i) {
    const int k = K - 1 - i;
    run_unet(h, s, k);
    const float* eps = (i < n_eps) ? z + (int64_t)(1 + i) * chw : nullptr;
    const float* nz = (!eps && noise_tail) ? noise_tail + (int64_t)(i - n_eps) * n : nullptr;
    a.geom.step = k; a.eps.p = eps;
    a.gauss.noise = nz; a.gauss.stream = (uint32_t)(0x1000 + i);
    launch_decode_step(h->st, sched_kind, a);
    if (k > range_t) {
      iv.qrow = k;
      iv.gauss.noise = ref_noise ? ref_noise + (int64_t)i * n : nullptr;
      iv.gauss.stream = (uint32_t)(0x5000 + i);  // its own stream: the step's draws are 0x1000 + i
      launch_ilvr_down(h->st, iv);
      launch_ilvr_up_add(h->st, iv);
    }
    h->pacer.tick(h->st);
  }
  HIP_CHECK(hipMemcpyAsync(x_out, s.xt, (size_t)n * 4, hipMemcpyDeviceToDevice, h->st));
  CD_API_END
}

}  // extern "C"

// ---- keep-mask estimation (csrc/automask.hip)
// the parameters cd_automask and cd_op_automask_reduce (capi_ops.hip) share, each refused by name
void check_sega_params(const cd_sega_concept* cp, int E, int64_t N, int K, float momentum_scale, float momentum_beta) {
  static_assert(sizeof(cd_sega_concept) == sizeof(SegaConcept), "concept ABI");
  const char* sg = "semantic guidance";
  CD_CHECK(E >= 1 && E <= kSegaMaxConcepts, "%s: E = %d concepts outside [1, %d]", sg, E, kSegaMaxConcepts);
  CD_CHECK(cp, "%s: concepts_host is NULL", sg);
  CD_CHECK(std::isfinite(momentum_scale), "%s: momentum_scale is not finite", sg);
  CD_CHECK(std::isfinite(momentum_beta) && momentum_beta >= 0.f && momentum_beta <= 1.f,
           "%s: momentum_beta = %g outside [0, 1]", sg, (double)momentum_beta);
  for (int e = 0; e < E; ++e) {
    CD_CHECK(std::isfinite(cp[e].scale), "%s: the scale of concept %d is not finite", sg, e);
    CD_CHECK(std::isfinite(cp[e].weight), "%s: the weight of concept %d is not finite", sg, e);
    CD_CHECK(cp[e].lo >= 0 && cp[e].lo <= N - 1, "%s: lo = %d of concept %d outside [0, N - 1 = %lld]", sg, cp[e].lo, e,
             (long long)(N - 1));
    CD_CHECK(cp[e].frac >= 0.f && cp[e].frac < 1.f, "%s: frac = %g of concept %d outside [0, 1)", sg, (double)cp[e].frac, e);
    CD_CHECK(cp[e].warm >= 0 && cp[e].warm <= cp[e].cool && (K < 0 || cp[e].cool <= K),
             "%s: warm = %d / cool = %d of concept %d outside 0 <= warm <= cool <= K (K = %d; negative: unbounded)", sg,
             cp[e].warm, cp[e].cool, e, K);
  }
}

void check_automask_params(int n_draws, float ratio, float thr, int dilate) {
  CD_CHECK(n_draws >= 1 && n_draws <= kStreamBandSteps, "keep-mask estimate: n_draws must lie in [1, %d] (the width of its stream "
                                                        "band), got %d", kStreamBandSteps, n_draws);
  CD_CHECK(ratio > 0.f, "keep-mask estimate: ratio must be > 0, got %g", (double)ratio);
  CD_CHECK(thr >= 0.f && thr < 1.f, "keep-mask estimate: thr must lie in [0, 1), got %g", (double)thr);
  CD_CHECK(dilate >= 0 && dilate <= kAutoMaskMaxDilate, "keep-mask estimate: dilate must lie in [0, %d], got %d",
           kAutoMaskMaxDilate, dilate);
}

extern "C" {

// The keep-mask of DiffEdit's first step: n_draws noised copies of x0 at one level, the network under the source and under the
// target context on each (one x_t per pair: the second half of the input is the copy of the first), and the reduction of
// automask.hip over |e_tgt - e_src|. The forward is cd_unet_forward's call on those rows; draws that do not fit max_rows rows
// run in further forwards and keep adding into the same per-pixel sums in draw order.
int cd_automask(cd_handle h, int net, const float* x0, const float* ctx_src, const float* ctx_tgt, int ctx_len, int B,
                int n_draws, int t, float qa, float qb, const float* noise, uint64_t seed, int max_rows, float ratio, float thr,
                int dilate, float* map_out, float* keep_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x0 && ctx_src && ctx_tgt && keep_out && B > 0 && ctx_len > 0, "bad argument");
  UNet* u = get_unet(h, net);
  CD_CHECK(u->kind() == CD_NET_UNET_OPENAI && u->desc.use_spatial_transformer && u->desc.context_dim > 0,
           "cd_automask: the estimate compares two text contexts; this network has no text context (a pixel network)");
  check_automask_params(n_draws, ratio, thr, dilate);
  CD_CHECK(max_rows >= 2 * B, "cd_automask: max_rows = %d holds no draw of a batch of %d (2 * B rows each)", max_rows, B);
  const int C = u->desc.in_channels, R = u->image_size, HW = R * R, Co = u->out_channels, Dc = u->desc.context_dim;
  CD_CHECK(Co == C, "cd_automask: the network predicts %d channels for %d input channels", Co, C);
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  AutoMaskArgs m;
  m.B = B; m.C = C; m.H = R; m.W = R;
  m.sb = (int64_t)HW * Co; m.sc = 1; m.sp = Co;  // the network's NHWC output
  m.n_total = n_draws; m.ratio = ratio; m.thr = thr; m.dilate = dilate;
  m.nblk = automask_sum_blocks(HW);
  m.acc = (float*)h->arena.alloc((size_t)B * HW * 4);
  m.partial = (float*)h->arena.alloc((size_t)B * m.nblk * 4);
  m.map_out = map_out; m.keep_out = keep_out;
  const size_t buffers = h->arena.mark();
  const int per_fwd = std::min(n_draws, std::max(1, max_rows / (2 * B)));
  const int64_t per_draw = (int64_t)B * C * HW;
  const size_t esz = u->f32 ? 4 : 2;
  AutoMaskNoised q;
  q.x0 = x0; q.qa = qa; q.qb = qb; q.seed = seed; q.B = B; q.C = C; q.HW = HW;
  bf16_t* xin = nullptr;
  float *eh = nullptr, *tvec = nullptr;
  int cur = 0;  // draws the buffers and the network's context are laid out for
  for (int i0 = 0; i0 < n_draws; i0 += per_fwd) {
    const int nc = std::min(per_fwd, n_draws - i0), rows = 2 * nc * B;
    if (nc != cur) {  // the first forward, and a shorter last one
      h->arena.release(buffers);
      bf16_t* cx = (bf16_t*)h->arena.alloc((size_t)rows * ctx_len * Dc * esz);
      for (int j = 0; j < 2 * nc; ++j)  // [c_src x nc | c_tgt x nc]
        put_ctx(h, u, j < nc ? ctx_src : ctx_tgt, cx, (size_t)j * B, B, ctx_len, Dc);
      u->set_context(c, cx, rows, ctx_len);
      xin = (bf16_t*)h->arena.alloc((size_t)rows * HW * u->in_cpad * esz);
      if (!u->f32) HIP_CHECK(hipMemsetAsync(xin, 0, (size_t)rows * HW * u->in_cpad * esz, h->st));  // the pad channels
      eh = (float*)h->arena.alloc((size_t)rows * HW * Co * 4);
      tvec = (float*)h->arena.alloc((size_t)rows * 4);
      launch_fill_f32(h->st, tvec, (float)t, rows);
      q.xq = u->f32 ? (float*)h->arena.alloc((size_t)nc * per_draw * 4) : nullptr;
      q.xin.xin = u->f32 ? nullptr : xin; q.xin.cpad = u->in_cpad; q.xin.dup = 1;
      cur = nc;
    }
    q.n_draws = nc;
    q.noise = noise ? noise + (int64_t)i0 * per_draw : nullptr;
    q.stream0 = (uint32_t)(0x6000 + i0);
    launch_automask_qsample(h->st, q);
    if (u->f32) put_net_input(h, u, q.xq, xin, nc * B, C, HW, u->in_cpad, 1.f, /*dup=*/true);  // the layout pass, once per half
    UNetIO io; io.xin = xin; io.B = rows; io.t_explicit = tvec; io.t_shared = false; io.out = eh; io.out_ld = Co;
    u->forward(c, io);
    m.e_src = eh; m.e_tgt = eh + (int64_t)nc * B * m.sb;
    m.n_chunk = nc; m.first = i0 == 0 ? 1 : 0;
    launch_automask_accum(h->st, m);
    h->pacer.tick(h->st);
  }
  launch_automask_finish(h->st, m);
  CD_API_END
}

// Per-word cross-attention heat maps: n_draws noised copies of x0 at one level through the CONDITIONAL forward
// only, every text cross-attention in the side window reduced by k_cross_attention_maps beside its own launch. A draw's layers
// add up inside its forward (per-row sums), the draws of a forward are then added to the call's sums in ascending order, so
// the result does not depend on how max_rows cuts the draws into forwards. The draws use the stream band 0x8000 + i: the
// band at 0x7000 holds the VAE posterior's stream 0x7a65.
int cd_word_maps(cd_handle h, int net, const float* x0, const float* ctx, int ctx_len, int B, const float* sel, int B_sel,
                 int N, int n_draws, int t, float qa, float qb, const float* noise, uint64_t seed, int max_rows,
                 int min_side, int max_side, float* maps_out, int* n_layers_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x0 && ctx && sel && maps_out && B > 0 && B_sel > 0 && ctx_len > 0, "bad argument");
  UNet* u = get_unet(h, net);
  CD_CHECK(u->kind() == CD_NET_UNET_OPENAI && u->desc.use_spatial_transformer && u->desc.context_dim > 0,
           "cd_word_maps: the maps are those of the text cross-attention; this network has no text context (a pixel network)");
  CD_CHECK(!u->f32, "cd_word_maps is not built for fp32 / fp32x3 networks (their transformer blocks run the fp32 attention of "
                    "st_f32.hip): use the 16-bit precision");
  CD_CHECK(ctx_len <= kCtrlKeys, "cd_word_maps: context length %d above the %d keys the kernel keeps resident", ctx_len,
           kCtrlKeys);
  CD_CHECK(N >= 1 && N <= kMapWords, "cd_word_maps: N = %d words outside [1, %d]", N, kMapWords);
  CD_CHECK(n_draws >= 1 && n_draws <= kStreamBandSteps, "cd_word_maps: n_draws must lie in [1, %d] (the width of its stream "
                                                        "band), got %d", kStreamBandSteps, n_draws);
  CD_CHECK(B % B_sel == 0, "cd_word_maps shape mismatch: %d selector entries for a batch of %d", B_sel, B);
  CD_CHECK(max_rows >= B, "cd_word_maps: max_rows = %d holds no draw of a batch of %d", max_rows, B);
  CD_CHECK(min_side >= 0 && min_side <= max_side, "cd_word_maps: side window [%d, %d] is empty (min_side > max_side)", min_side,
           max_side);
  const int n_layers = u->count_text_blocks(min_side, max_side);
  CD_CHECK(n_layers > 0, "cd_word_maps: no transformer block has a token grid side in [%d, %d]", min_side, max_side);
  const int C = u->desc.in_channels, R = u->image_size, HW = R * R, Co = u->out_channels, Dc = u->desc.context_dim;
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  const int64_t per_map = (int64_t)N * HW;
  float* total = (float*)h->arena.alloc((size_t)B * per_map * 4);
  const size_t buffers = h->arena.mark();
  const int per_fwd = std::min(n_draws, std::max(1, max_rows / B));
  const int64_t per_draw = (int64_t)B * C * HW;
  AutoMaskNoised q;
  q.x0 = x0; q.qa = qa; q.qb = qb; q.seed = seed; q.B = B; q.C = C; q.HW = HW;
  WordMapCollect wm;
  wm.sel = sel; wm.N = N; wm.B_sel = B_sel; wm.min_side = min_side; wm.max_side = max_side; wm.B = B;
  bf16_t* xin = nullptr;
  float *eh = nullptr, *tvec = nullptr;
  int cur = 0;  // draws the buffers and the network's context are laid out for
  for (int i0 = 0; i0 < n_draws; i0 += per_fwd) {
    const int nc = std::min(per_fwd, n_draws - i0), rows = nc * B;
    if (nc != cur) {  // the first forward, and a shorter last one
      h->arena.release(buffers);
      bf16_t* cx = (bf16_t*)h->arena.alloc((size_t)rows * ctx_len * Dc * 2);
      for (int j = 0; j < nc; ++j) put_ctx(h, u, ctx, cx, (size_t)j * B, B, ctx_len, Dc);  // the context once per draw
      u->set_context(c, cx, rows, ctx_len);
      xin = (bf16_t*)h->arena.alloc((size_t)rows * HW * u->in_cpad * 2);
      HIP_CHECK(hipMemsetAsync(xin, 0, (size_t)rows * HW * u->in_cpad * 2, h->st));  // the pad channels
      eh = (float*)h->arena.alloc((size_t)rows * HW * Co * 4);
      tvec = (float*)h->arena.alloc((size_t)rows * 4);
      launch_fill_f32(h->st, tvec, (float)t, rows);
      wm.acc = (float*)h->arena.alloc((size_t)rows * per_map * 4);
      q.xin.xin = xin; q.xin.cpad = u->in_cpad; q.xin.dup = 0;
      cur = nc;
    }
    q.n_draws = nc;
    q.noise = noise ? noise + (int64_t)i0 * per_draw : nullptr;
    q.stream0 = (uint32_t)(0x8000 + i0);
    launch_automask_qsample(h->st, q);
    wm.n_chunk = nc;
    UNetIO io; io.xin = xin; io.B = rows; io.t_explicit = tvec; io.t_shared = false; io.out = eh; io.out_ld = Co;
    io.maps = &wm;
    u->forward(c, io);
    CD_CHECK(wm.layers == n_layers, "cd_word_maps: the forward collected %d blocks of %d", wm.layers, n_layers);
    WordMapFold f;
    f.acc = wm.acc; f.total = total; f.n_chunk = nc; f.B = B; f.per = per_map; f.first = i0 == 0 ? 1 : 0;
    if (i0 + nc == n_draws) { f.out = maps_out; f.scale = 1.0f / (float)(n_draws * n_layers); }
    launch_word_map_fold(h->st, f);
    h->pacer.tick(h->st);
  }
  if (n_layers_out) *n_layers_out = n_layers;
  CD_API_END
}

}  // extern "C"

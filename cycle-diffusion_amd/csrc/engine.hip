// Arena, parameter store and the shared building blocks (conv / norm / attention wrappers).
#include <limits.h>
#include <stdlib.h>

#include "engine.h"

#include <string.h>

namespace cd {

// ------------------------------------------------------------------ Arena
Arena::~Arena() { if (base_) (void)hipFree(base_); }
void Arena::init(size_t bytes) {
  if (base_) { (void)hipFree(base_); base_ = nullptr; }
  HIP_CHECK(hipMalloc((void**)&base_, bytes));
  cap_ = bytes; off_ = 0; high_ = 0;
}
void* Arena::alloc(size_t bytes) {
  size_t a = (off_ + 255) & ~(size_t)255;
  CD_CHECK(a + bytes <= cap_, "workspace arena exhausted: need %zu more bytes (capacity %zu); "
           "create the engine with a larger workspace", a + bytes - cap_, cap_);
  off_ = a + bytes;
  if (off_ > high_) high_ = off_;
  return base_ + a;
}

// ------------------------------------------------------------------ ParamStore
ParamStore::~ParamStore() {
  for (void* p : allocs_) (void)hipFree(p);
  if (staging_) (void)hipFree(staging_);
}
void* ParamStore::dmalloc(size_t bytes) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes < 256 ? 256 : bytes));
  HIP_CHECK(hipMemset(p, 0, bytes < 256 ? 256 : bytes));
  allocs_.push_back(p);
  dev_bytes_ += bytes;
  return p;
}
ConvW* ParamStore::new_conv(int N, int Cin, int KH, int KW, bool bias, bool geglu) {
  convs_.emplace_back(new ConvW());
  ConvW* c = convs_.back().get();
  c->N = N; c->Cin = Cin; c->KH = KH; c->KW = KW; c->geglu = geglu;
  c->Cpad = round_up(Cin, 32);
  c->Npad = round_up(N, 128);
  c->f32 = f32;
  c->w = (bf16_t*)dmalloc((size_t)c->Npad * c->Ktot() * (f32 ? sizeof(float) : sizeof(bf16_t)));
  if (!f32 && KH == 1 && KW == 1 && c->Cpad == 320)  // the streaming linear kernel reads fragment-major weights
    c->wfrag = (bf16_t*)dmalloc((size_t)c->Npad * c->Cpad * sizeof(bf16_t));
  if (f32 && x3) c->w3 = (bf16_t*)dmalloc((size_t)c->Npad * c->Ktot() * 3 * sizeof(bf16_t));
  if (bias) c->b = (float*)dmalloc((size_t)c->Npad * sizeof(float));
  return c;
}
void ParamStore::add_up_phase(ConvW* c) {
  if (f32 || c->wphase || c->KH != 3 || c->KW != 3 || c->geglu) return;
  c->wphase = (bf16_t*)dmalloc((size_t)4 * c->Npad * 4 * c->Cpad * sizeof(bf16_t));
  c->wphase_version = -1;
}
void ParamStore::refresh_up_phase(hipStream_t st, ConvW* c) {
  if (!c->wphase || c->wphase_version == version) return;
  launch_up_phase_weights(st, c->w, c->wphase, c->Npad, c->Cpad);
  c->wphase_version = version;
}
float* ParamStore::new_vec(int n, float init) {
  float* p = (float*)dmalloc((size_t)n * sizeof(float));
  if (init != 0.f) {
    std::vector<float> h(n, init);
    HIP_CHECK(hipMemcpy(p, h.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  }
  return p;
}
ParamDecl& ParamStore::declare(const std::string& name, std::vector<int64_t> shape) {
  auto it = by_name_.find(name);
  if (it != by_name_.end()) {
    CD_CHECK(it->second->shape == shape, "parameter %s declared twice with different shapes", name.c_str());
    return *it->second;
  }
  decls_.emplace_back(new ParamDecl());
  ParamDecl* d = decls_.back().get();
  d->name = name; d->shape = std::move(shape);
  by_name_[name] = d;
  return *d;
}
void ParamStore::conv_weight(const std::string& name, ConvW* c, int ref_ndim, float scale) {
  std::vector<int64_t> shape;
  if (ref_ndim == 0) ref_ndim = (c->KH == 1 && c->KW == 1) ? 2 : 4;
  if (ref_ndim == 2) shape = {c->N, c->Cin};
  else if (ref_ndim == 3) shape = {c->N, c->Cin, 1};
  else shape = {c->N, c->Cin, c->KH, c->KW};
  ParamDecl& d = declare(name, shape);
  PackTarget t; t.kind = PackTarget::MATRIX_BF16; t.conv = c; t.dst_row0 = 0; t.rows = c->N;
  t.src_base = 0; t.grp = c->N; t.grp_stride = 0; t.geglu = c->geglu; t.scale = scale;
  d.targets.push_back(t);
}
void ParamStore::conv_weight_t(const std::string& name, ConvW* c) {
  CD_CHECK(c->KH == 1 && c->KW == 1, "transposed weights are linear layers");
  ParamDecl& d = declare(name, {c->Cin, c->N});
  d.transposed = true;
  PackTarget t; t.kind = PackTarget::MATRIX_BF16; t.conv = c; t.dst_row0 = 0; t.rows = c->N;
  t.src_base = 0; t.grp = c->N; t.grp_stride = 0; t.geglu = false;
  d.targets.push_back(t);
}
void ParamStore::conv_bias(const std::string& name, ConvW* c) {
  CD_CHECK(c->b, "conv %s has no bias storage", name.c_str());
  ParamDecl& d = declare(name, {c->N});
  PackTarget t; t.kind = PackTarget::VECTOR_F32; t.fdst = c->b; t.dst_off = 0; t.rows = c->N;
  t.src_base = 0; t.grp = c->N; t.grp_stride = 0; t.geglu = c->geglu; t.geglu_N = c->N;
  d.targets.push_back(t);
}
void ParamStore::conv_rows(const std::string& name, std::vector<int64_t> shape, ConvW* c, int dst_row0,
                           int rows, int src_base, int grp, int grp_stride, float scale) {
  ParamDecl& d = declare(name, std::move(shape));
  PackTarget t; t.kind = PackTarget::MATRIX_BF16; t.conv = c; t.dst_row0 = dst_row0; t.rows = rows;
  t.src_base = src_base; t.grp = grp; t.grp_stride = grp_stride; t.scale = scale;
  d.targets.push_back(t);
}
void ParamStore::bias_rows(const std::string& name, int64_t n_total, float* dst, int dst_off, int rows,
                           int src_base, int grp, int grp_stride) {
  ParamDecl& d = declare(name, {n_total});
  PackTarget t; t.kind = PackTarget::VECTOR_F32; t.fdst = dst; t.dst_off = dst_off; t.rows = rows;
  t.src_base = src_base; t.grp = grp; t.grp_stride = grp_stride;
  d.targets.push_back(t);
}
void ParamStore::vec(const std::string& name, float* dst, int n) {
  bias_rows(name, n, dst, 0, n, 0, n, 0);
}
void ParamStore::mat_f32(const std::string& name, float* dst, int N, int K, int dst_row0) {
  ParamDecl& d = declare(name, {N, K});
  PackTarget t; t.kind = PackTarget::MATRIX_F32; t.fdst = dst; t.dst_off = dst_row0; t.rows = N; t.K = K;
  t.src_base = 0; t.grp = N; t.grp_stride = 0;
  d.targets.push_back(t);
}

// repack with a row map: dst row j <- src row src_base + (j/grp)*grp_stride + j%grp
template <typename OutT>
__global__ void k_pack_rows(const float* __restrict__ w, OutT* __restrict__ out, int rows, int Cin,
                            int KH, int KW, int Cpad, int dst_row0, int src_base, int grp,
                            int grp_stride, int geglu, int Ntot, float scale) {
  const int64_t total = (int64_t)rows * KH * KW * Cpad;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cpad);
    int64_t t = i / Cpad;
    const int s = (int)(t % KW); t /= KW;
    const int r = (int)(t % KH); t /= KH;
    const int j = (int)t;  // destination row (relative)
    int jj = j;
    if (geglu) {  // packed row j: blocks of 64 = [32 value | 32 gate]
      const int blk = j / 64, within = j % 64;
      jj = (within < 32) ? blk * 32 + within : Ntot / 2 + blk * 32 + (within - 32);
    }
    const int src = src_base + (jj / grp) * grp_stride + (jj % grp);
    float v = 0.f;
    if (c < Cin) v = w[(((int64_t)src * Cin + c) * KH + r) * KW + s] * scale;
    const int64_t o = ((int64_t)(dst_row0 + j) * KH * KW + (int64_t)r * KW + s) * Cpad + c;
    if constexpr (sizeof(OutT) == 4) out[o] = v;
    else out[o] = f2bf(v);
  }
}

void ParamStore::load(hipStream_t st, const std::string& name, const float* host, int ndim,
                      const int64_t* shape) {
  ++version;
  auto it = by_name_.find(name);
  CD_CHECK(it != by_name_.end(), "unknown parameter name '%s'", name.c_str());
  ParamDecl& d = *it->second;
  int64_t n = 1, nd = 1;
  for (int i = 0; i < ndim; ++i) n *= shape[i];
  for (auto s : d.shape) nd *= s;
  // accept [N,C] for [N,C,1,1] / [N,C,1] (conv1d / 1x1 conv stored as linear and vice versa)
  bool ok = (n == nd) && ndim >= 1 && shape[0] == d.shape[0];
  if (ok && d.shape.size() >= 2 && ndim >= 2) ok = (shape[1] == d.shape[1]);
  CD_CHECK(ok, "parameter %s: shape mismatch (got %lld elements, ndim %d; expected %lld)", name.c_str(),
           (long long)n, ndim, (long long)nd);
  const size_t bytes = (size_t)n * sizeof(float);
  if (bytes > staging_bytes_) {
    if (staging_) HIP_CHECK(hipFree(staging_));
    staging_bytes_ = bytes < (1u << 20) ? (1u << 20) : bytes;
    HIP_CHECK(hipMalloc((void**)&staging_, staging_bytes_));
  }
  HIP_CHECK(hipStreamSynchronize(st));
  if (d.transposed) {  // [K][N] -> [N][K] on the host (small projection matrices)
    const int64_t K = d.shape[0], N = d.shape[1];
    std::vector<float> tr((size_t)n);
    for (int64_t k = 0; k < K; ++k)
      for (int64_t j = 0; j < N; ++j) tr[(size_t)j * K + k] = host[(size_t)k * N + j];
    HIP_CHECK(hipMemcpy(staging_, tr.data(), bytes, hipMemcpyHostToDevice));
  } else {
    HIP_CHECK(hipMemcpy(staging_, host, bytes, hipMemcpyHostToDevice));
  }
  for (const PackTarget& t : d.targets) {
    if (t.kind == PackTarget::MATRIX_BF16) {
      const ConvW* c = t.conv;
      const int64_t total = (int64_t)t.rows * c->KH * c->KW * c->Cpad;
      int grid = (int)((total + 255) / 256);
      if (grid > 8192) grid = 8192;
      if (c->f32)
        hipLaunchKernelGGL(k_pack_rows<float>, dim3(grid), dim3(256), 0, st, staging_, (float*)c->w, t.rows, c->Cin,
                           c->KH, c->KW, c->Cpad, t.dst_row0, t.src_base, t.grp, t.grp_stride, t.geglu ? 1 : 0, c->N,
                           t.scale);
      else
        hipLaunchKernelGGL(k_pack_rows<bf16_t>, dim3(grid), dim3(256), 0, st, staging_, c->w, t.rows, c->Cin, c->KH,
                           c->KW, c->Cpad, t.dst_row0, t.src_base, t.grp, t.grp_stride, t.geglu ? 1 : 0, c->N, t.scale);
      if (c->wfrag) launch_pack_wfrag(st, c->w, c->Ktot(), c->wfrag, c->Npad);  // whole matrix: rows may come in parts
      if (c->w3) launch_pack_w3(st, (const float*)c->w, c->w3, c->Npad, c->KH * c->KW, c->Cpad, overflow);
    } else {
      // small: map on the host
      const int K = (t.kind == PackTarget::MATRIX_F32) ? t.K : 1;
      std::vector<float> tmp((size_t)t.rows * K);
      for (int j = 0; j < t.rows; ++j) {
        int jj = j;
        if (t.geglu) {
          const int blk = j / 64, within = j % 64;
          jj = (within < 32) ? blk * 32 + within : t.geglu_N / 2 + blk * 32 + (within - 32);
        }
        const int src = t.src_base + (jj / t.grp) * t.grp_stride + (jj % t.grp);
        memcpy(&tmp[(size_t)j * K], host + (size_t)src * K, (size_t)K * sizeof(float));
      }
      HIP_CHECK(hipMemcpy(t.fdst + (size_t)t.dst_off * K, tmp.data(), tmp.size() * sizeof(float),
                          hipMemcpyHostToDevice));
    }
  }
  HIP_CHECK(hipStreamSynchronize(st));
  d.loaded = true;
}

int ParamStore::missing(std::string* first) const {
  int n = 0;
  for (auto& d : decls_)
    if (!d->loaded) {
      if (n == 0 && first) *first = d->name;
      ++n;
    }
  return n;
}

// ------------------------------------------------------------------ building blocks
Act alloc_act(Ctx& c, int B, int H, int W, int C, bool with_stats) {
  Act a; a.B = B; a.H = H; a.W = W; a.C = C; a.ld = C; a.f32 = c.f32;
  a.p = (bf16_t*)c.arena->alloc((size_t)B * H * W * C * (c.f32 ? sizeof(float) : sizeof(bf16_t)));
  if ((!c.f32 || c.x3) && with_stats && ((H * W) % 32) == 0)  // fp32 path: only its split mode emits statistics
    a.stats_buf = (float*)c.arena->alloc((size_t)(B * H * W / 32) * 2 * C * sizeof(float));
  return a;
}

// CD_PREC_F32X3: x = [hi | lo] fp16 pairs (a GroupNorm output), weights [wh | wh | wl]: one 16-bit implicit GEMM
// over the channel list [hi | lo | hi], fp32 bias / time-embedding row / residual / output (kernels.h kX3ActScale)
static Act conv_split_fwd(Ctx& c, const ConvW& w, const Act& x, const ConvOpts& o) {
  CD_CHECK(c.f32 && c.x3 && w.w3 && (!w.geglu || o.raw_geglu), "conv: split input outside the split-fp16 mode");
  CD_CHECK(x.C == w.Cpad && x.ld == 2 * x.C, "conv: split input of %d channels (ld %d) against Cpad %d", x.C, x.ld, w.Cpad);
  CD_CHECK(!o.ln_fold && (!o.resid || (o.resid->f32 && !o.resid->split)), "conv: split-mode operands");
  ConvGemmParams p;
  p.src0 = x.p; p.C0 = 2 * x.C; p.ld0 = x.ld;
  p.src1 = x.p; p.C1 = x.C; p.ld1 = x.ld;
  p.B = x.B; p.Hs = x.H; p.Ws = x.W; p.up = o.up ? 1 : 0;
  p.Hin = o.up ? x.H * 2 : x.H; p.Win = o.up ? x.W * 2 : x.W;
  p.KH = w.KH; p.KW = w.KW; p.stride = o.stride;
  if (o.asym) { p.pad_t = 0; p.pad_l = 0; p.Hout = (p.Hin + 1 - w.KH) / o.stride + 1; p.Wout = (p.Win + 1 - w.KW) / o.stride + 1; }
  else {
    p.pad_t = o.pad; p.pad_l = o.pad;
    p.Hout = (p.Hin + 2 * o.pad - w.KH) / o.stride + 1;
    p.Wout = (p.Win + 2 * o.pad - w.KW) / o.stride + 1;
  }
  p.M = x.B * p.Hout * p.Wout;
  p.wgt = w.w3; p.Ktot = 3 * w.Ktot(); p.N = w.N;
  p.alpha = o.alpha * (1.0f / (kX3ActScale * kX3WgtScale)); p.bias = w.b;
  p.rowvec = o.rowvec; p.rowvec_ld = o.rowvec_ld; p.rows_per_vec = o.rows_per_vec;
  p.act = o.act;
  Act y; y.B = x.B; y.H = p.Hout; y.W = p.Wout; y.C = w.N; y.f32 = true;
  if (o.out) { y.p = (bf16_t*)o.out; y.ld = o.out_ld; }
  else { y.ld = w.N; y.p = (bf16_t*)c.arena->alloc((size_t)p.M * w.N * 4); }
  if (o.resid) {
    CD_CHECK(o.resid->rows() == p.M && o.resid->C == w.N, "conv: residual shape mismatch");
    p.resid = o.resid->p; p.resid_ld = o.resid->ld; p.resid_f32 = 1;
  }
  p.out = y.p; p.out_ld = y.ld; p.out_f32 = 1;
  p.zeros = c.zeros; p.tile = o.tile;
  p.prof_flop_scale = 1.0f / 3.0f;
  if (((p.Hout * p.Wout) % 32) == 0) {  // the consumer's GroupNorm statistics from the epilogue, as on the 16-bit path
    if (o.out && o.out_stats) y.stats_buf = o.out_stats;
    else if (!o.out && o.want_stats)
      y.stats_buf = (float*)c.arena->alloc((size_t)(p.M / 32) * 2 * w.N * sizeof(float));
    p.stats = y.stats_buf;
    y.stats = y.stats_buf;
  }
  launch_conv_gemm(c.st, p);
  return y;
}

// Phase form of the nearest-x2 3 x 3 convs: 4/9 of the multiply-adds. Taken where the weights carry their
// phase matrices (the U-Net Upsample layers), the stored image is a multiple of 256 pixels (a tile then lies in one phase of
// one image: 16 x 16 and larger) and the epilogue needs nothing per output position (no residual). CYCLEDIFF_UP_PHASE=0
// keeps the x2 gather for A/B runs; read per call (three convs a forward), so a process can run both.
bool conv_up_phase_taken(const Ctx& c, const ConvW& w, const Act& x, const Act* x2, const ConvOpts& o) {
  if (!o.up || c.f32 || x.split || x2 || !w.wphase || w.KH != 3 || w.KW != 3 || o.stride != 1 || o.pad != 1 || o.asym ||
      o.resid || o.out_f32 || o.ln_fold || w.geglu || o.act != ACT_NONE)
    return false;
  if ((x.H * x.W) % 256 != 0 || w.N % 8 != 0 || (o.out && o.out_ld % 8 != 0)) return false;
  const char* e = getenv("CYCLEDIFF_UP_PHASE");
  return !(e && e[0] == '0');
}

static Act conv_up_phase_fwd(Ctx& c, const ConvW& w, const Act& x, const ConvOpts& o) {
  ConvGemmParams p;
  p.src0 = x.p; p.C0 = round_up(x.C, 32); p.ld0 = x.ld;
  CD_CHECK(p.C0 == w.Cpad && x.ld >= p.C0, "conv: input channels %d do not match weight Cpad %d", p.C0, w.Cpad);
  p.B = x.B; p.Hs = x.H; p.Ws = x.W; p.Hin = x.H; p.Win = x.W; p.Hout = x.H; p.Wout = x.W;
  p.KH = 2; p.KW = 2; p.stride = 1; p.pad_t = 1; p.pad_l = 1;  // (the kernel takes the padding from the tile's phase)
  p.up_phase = 1; p.w_ps = w.Npad * 4 * w.Cpad;
  p.M = 4 * x.B * x.H * x.W;
  p.wgt = w.wphase; p.Ktot = 4 * w.Cpad; p.N = w.N;
  p.alpha = o.alpha; p.bias = w.b;
  p.rowvec = o.rowvec; p.rowvec_ld = o.rowvec_ld; p.rows_per_vec = o.rows_per_vec;  // per image: its 4 H W rows stay together
  Act y; y.B = x.B; y.H = 2 * x.H; y.W = 2 * x.W; y.C = w.N; y.f32 = false;
  if (o.out) { y.p = (bf16_t*)o.out; y.ld = o.out_ld; }
  else { y.ld = w.N; y.p = (bf16_t*)c.arena->alloc((size_t)p.M * w.N * 2); }
  if (o.out && o.out_stats) y.stats_buf = o.out_stats;
  else if (!o.out && o.want_stats) y.stats_buf = (float*)c.arena->alloc((size_t)(p.M / 32) * 2 * w.N * sizeof(float));
  p.stats = y.stats_buf;  // 32-row blocks in phase order: an image's blocks are still its own, which is all k_gn_fold asks
  y.stats = y.stats_buf;
  const size_t mk = c.arena->mark();
  bf16_t* tmp = (bf16_t*)c.arena->alloc((size_t)p.M * w.N * 2);  // rows in (image, phase, y, x) order
  p.out = tmp; p.out_ld = w.N;
  p.zeros = c.zeros; p.tile = o.tile;
  launch_conv_gemm(c.st, p);
  launch_up_phase_reorder(c.st, tmp, y.p, x.B, x.H, x.W, w.N, y.ld);
  c.arena->release(mk);
  return y;
}

Act conv_fwd(Ctx& c, const ConvW& w, const Act& x, const Act* x2, const ConvOpts& o) {
  if (conv_up_phase_taken(c, w, x, x2, o)) return conv_up_phase_fwd(c, w, x, o);
  if (x.split) {
    CD_CHECK(!x2, "conv: a split activation cannot be concatenated");
    return conv_split_fwd(c, w, x, o);
  }
  ConvGemmParams p;
  CD_CHECK(w.f32 == c.f32 && x.f32 == c.f32 && (!x2 || x2->f32 == c.f32) && (!o.resid || o.resid->f32 == c.f32),
           "conv: operand precision does not match the running network");
  CD_CHECK((!x2 || !x2->split) && (!o.resid || !o.resid->split), "conv: split activation as a second source / residual");
  p.src0 = x.p; p.C0 = round_up(x.C, 32); p.ld0 = x.ld;
  if (x2) {
    CD_CHECK(x2->B == x.B && x2->H == x.H && x2->W == x.W, "conv: concat sources differ in shape");
    p.src1 = x2->p; p.C1 = x2->C; p.ld1 = x2->ld;
    CD_CHECK(x.C % 32 == 0 && x2->C % 32 == 0, "conv: concat channels must be multiples of 32");
  }
  CD_CHECK(p.C0 + p.C1 == w.Cpad, "conv: input channels %d+%d do not match weight Cpad %d", p.C0, p.C1, w.Cpad);
  CD_CHECK(x.ld >= p.C0, "conv: source row shorter than padded channel count");
  p.B = x.B; p.Hs = x.H; p.Ws = x.W; p.up = o.up ? 1 : 0;
  p.Hin = o.up ? x.H * 2 : x.H; p.Win = o.up ? x.W * 2 : x.W;
  p.KH = w.KH; p.KW = w.KW; p.stride = o.stride;
  if (o.asym) { p.pad_t = 0; p.pad_l = 0; p.Hout = (p.Hin + 1 - w.KH) / o.stride + 1; p.Wout = (p.Win + 1 - w.KW) / o.stride + 1; }
  else {
    p.pad_t = o.pad; p.pad_l = o.pad;
    p.Hout = (p.Hin + 2 * o.pad - w.KH) / o.stride + 1;
    p.Wout = (p.Win + 2 * o.pad - w.KW) / o.stride + 1;
  }
  p.M = x.B * p.Hout * p.Wout;
  p.wgt = w.w; p.wgt_frag = w.wfrag; p.Ktot = w.Ktot(); p.N = w.N;
  p.alpha = o.alpha; p.bias = w.b;
  p.rowvec = o.rowvec; p.rowvec_ld = o.rowvec_ld; p.rows_per_vec = o.rows_per_vec;
  const bool fuse_geglu = w.geglu && !o.raw_geglu;
  p.act = fuse_geglu ? ACT_GEGLU : o.act;
  const int Nout = fuse_geglu ? w.N / 2 : w.N;
  Act y; y.B = x.B; y.H = p.Hout; y.W = p.Wout; y.C = Nout; y.f32 = c.f32;
  if (o.out) { y.p = (bf16_t*)o.out; y.ld = o.out_ld; }
  else {
    y.ld = Nout;
    y.p = (bf16_t*)c.arena->alloc((size_t)p.M * Nout * ((o.out_f32 || c.f32) ? 4 : 2));
  }
  if (o.resid) {
    CD_CHECK(o.resid->rows() == p.M && o.resid->C == Nout, "conv: residual shape mismatch");
    p.resid = o.resid->p; p.resid_ld = o.resid->ld;
  }
  p.out = y.p; p.out_ld = y.ld; p.out_f32 = o.out_f32 ? 1 : 0;
  p.zeros = c.zeros; p.tile = o.tile;
  if (o.ln_fold) { p.ln_fold = 1; p.ln_eps = o.ln_eps; p.tile = kLinStreamTile; }
  if (c.f32) {
    p.out_f32 = 1;
    launch_conv_gemm_f32(c.st, p);
    return y;
  }
  if (!w.geglu && !o.out_f32 && ((p.Hout * p.Wout) % 32) == 0) {
    if (o.out && o.out_stats) y.stats_buf = o.out_stats;
    else if (!o.out && o.want_stats)
      y.stats_buf = (float*)c.arena->alloc((size_t)(p.M / 32) * 2 * Nout * sizeof(float));
    p.stats = y.stats_buf;
    y.stats = y.stats_buf;
  }
  launch_conv_gemm(c.st, p);
  return y;
}

bool conv_ln_fold_available(const Ctx& c, const ConvW& w, int64_t rows) {
  static const bool on = [] { const char* e = getenv("CYCLEDIFF_LN_FOLD"); return !(e && e[0] == '0'); }();  // A/B runs
  // the streaming kernel owns 256-row strips, one persistent workgroup per CU: below ~3/4 of the CUs' worth of strips the
  // tile kernel + a LayerNorm launch is the better pair (CYCLEDIFF_LN_FOLD_MIN_ROWS overrides the threshold for A/B runs)
  static const int64_t min_rows = [] { const char* e = getenv("CYCLEDIFF_LN_FOLD_MIN_ROWS"); return e ? atoll(e) : 32768ll; }();
  return on && !c.f32 && w.wfrag && w.KH == 1 && w.KW == 1 && w.Cpad == 320 && rows >= min_rows && rows % 32 == 0 &&
         w.N % 64 == 0 && w.N <= 2560;
}

Act groupnorm_fwd(Ctx& c, const GNW& w, const Act& x, const Act* x2, bool silu, const float* film,
                  int film_ld) {
  GroupNormParams p;
  p.x = x.p; p.C0 = x.C; p.ld0 = x.ld;
  if (x2) { p.x1 = x2->p; p.C1 = x2->C; p.ld1 = x2->ld; }
  const int C = p.C0 + p.C1;
  CD_CHECK(C == w.C, "groupnorm: channels %d != weight %d", C, w.C);
  p.B = x.B; p.HW = x.H * x.W; p.G = 32; p.eps = w.eps; p.gamma = w.g; p.beta = w.b;
  p.film = film; p.film_ld = film_ld; p.silu = silu ? 1 : 0;
  Act y = alloc_act(c, x.B, x.H, x.W, C);
  p.y = y.p;
  if (c.f32) {
    CD_CHECK(x.f32 && (!x2 || x2->f32) && !x.split && (!x2 || !x2->split), "groupnorm: operand precision");
    if (c.x3) { p.split_out = 1; p.overflow = c.overflow; y.split = true; y.ld = 2 * C; }  // same bytes as the fp32 tensor
    if (x.stats && x.ld == x.C && (!x2 || (x2->stats && x2->ld == x2->C))) {  // written by the split convs' epilogues
      p.pre0 = x.stats;
      p.pre1 = x2 ? x2->stats : nullptr;
    }
    const size_t mk = c.arena->mark();
    void* ws = c.arena->alloc(groupnorm_f32_workspace(p.B, p.HW, C));
    launch_groupnorm_f32(c.st, p, ws);
    c.arena->release(mk);  // stream order keeps the scratch alive until the three kernels have run
    return y;
  }
  p.S = groupnorm_slabs(p.B, p.HW, C);
  const size_t part_floats = round_up((size_t)p.B * p.S * p.G * 2, (size_t)64);
  CD_CHECK(part_floats + (size_t)p.B * 2 * C <= c.gn_partial_floats, "groupnorm: workspace too small");
  p.partial = c.gn_partial;
  p.coef = c.gn_partial + part_floats;
  if (x.stats && x.ld == x.C && (!x2 || (x2->stats && x2->ld == x2->C))) {
    p.pre0 = x.stats;
    p.pre1 = x2 ? x2->stats : nullptr;
  }
  launch_groupnorm(c.st, p);
  return y;
}

const float* groupnorm_coef_fwd(Ctx& c, const GNW& w, const Act& x) {
  CD_CHECK(!c.f32 && !x.f32 && !x.split && x.C == w.C, "groupnorm coefficients: 16-bit single source of %d channels", w.C);
  GroupNormParams p;
  p.x = x.p; p.C0 = x.C; p.ld0 = x.ld;
  p.B = x.B; p.HW = x.H * x.W; p.G = 32; p.eps = w.eps; p.gamma = w.g; p.beta = w.b;
  p.no_apply = 1;
  p.S = groupnorm_slabs(p.B, p.HW, x.C);
  const size_t part_floats = round_up((size_t)p.B * p.S * p.G * 2, (size_t)64);
  CD_CHECK(part_floats + (size_t)p.B * 2 * x.C <= c.gn_partial_floats, "groupnorm: workspace too small");
  p.partial = c.gn_partial;
  p.coef = c.gn_partial + part_floats;
  if (x.stats && x.ld == x.C) p.pre0 = x.stats;
  launch_groupnorm(c.st, p);
  return p.coef;
}

// ------------------------------------------------------------------ entry of the 64 x 64 transformer blocks
int st_entry_stages() {
  static const int v = [] {
    const char* e = getenv("CYCLEDIFF_ST_ENTRY");
    int s = e && e[0] ? atoi(e) : (ST_ENTRY_QKV | ST_ENTRY_LN1 | ST_ENTRY_GN);
    if (!(s & ST_ENTRY_QKV)) s &= ~ST_ENTRY_LN1;
    return s;
  }();
  return v;
}

bool st_entry_available(const Ctx& c, int64_t rows, int hw) {
  // whole images per 256-row strip, and at least half a round of the chip's CUs in strips: below that the persistent
  // workgroups of the streaming kernel leave most of the chip idle. (Where the U-Net takes the launches is its own,
  // narrower choice: kStEntryNetMinRows.)
  return !c.f32 && rows >= 32768 && lin_stream_entry_supports(rows, hw, 320);
}

void st_entry_alloc(ParamStore& ps, StEntryW& w) {
  if (!w.qk1 || !w.v1 || !w.qk1->wfrag || !w.v1->wfrag || w.qk1->Cpad != 320 || w.qk1->N != 640 || w.v1->N != 320) return;
  w.qkv = ps.new_conv(960, 320, 1, 1, true);
  w.qkv_ln = ps.new_conv(960, 320, 1, 1, true);
}

void st_entry_refresh(hipStream_t st, StEntryW& w) {
  if (!w.qkv) return;
  const size_t row = (size_t)320 * sizeof(bf16_t);
  HIP_CHECK(hipMemcpyAsync(w.qkv->w, w.qk1->w, 640 * row, hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipMemcpyAsync(w.qkv->w + (size_t)640 * 320, w.v1->w, 320 * row, hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipMemsetAsync(w.qkv->b, 0, 960 * sizeof(float), st));
  if (w.vbias) HIP_CHECK(hipMemcpyAsync(w.qkv->b + 640, w.vbias, 320 * sizeof(float), hipMemcpyDeviceToDevice, st));
  launch_pack_wfrag(st, w.qkv->w, 320, w.qkv->wfrag, 960);
  if (w.ln1.g && w.qkv_ln) {
    launch_fold_ln(st, w.qkv->w, 320, w.ln1.g, w.ln1.b, w.qkv->b, w.qkv_ln->w, w.qkv_ln->b, 960, 320);
    launch_pack_wfrag(st, w.qkv_ln->w, 320, w.qkv_ln->wfrag, 960);
  }
}

// V^T[b] = Wv . X[b]^T : weights as the A operand, tokens as the B operand -> [B][C][Tpad]
void vt_gemm_fwd(Ctx& c, const ConvW& wv, const bf16_t* x, int ldx, int B, int T, int Tpad, bf16_t* vt) {
  ConvGemmParams p;
  p.src0 = wv.w; p.C0 = wv.Cpad; p.ld0 = wv.Cpad;
  p.B = 1; p.Hs = wv.N; p.Ws = 1; p.Hin = wv.N; p.Win = 1; p.Hout = wv.N; p.Wout = 1;
  p.M = wv.N;
  p.wgt = x; p.Ktot = wv.Cpad; p.ldw = ldx; p.N = T;
  p.nbatch = B; p.a_bs = 0; p.w_bs = (int64_t)T * ldx; p.o_bs = (int64_t)wv.N * Tpad;
  p.out = vt; p.out_ld = Tpad; p.zeros = c.zeros;
  launch_conv_gemm(c.st, p);
}

int st_entry_effective(const Ctx& c, const StEntryW& w, const Act& x, int stages) {
  const bool fused_ok = w.qkv && w.norm.C == 320 && x.C == 320 && x.ld == 320 && st_entry_available(c, x.rows(), x.H * x.W);
  if (!fused_ok) stages = 0;
  // norm1 folds where norm2 / norm3 do (CYCLEDIFF_LN_FOLD, its row threshold), and only into the q | k | v launch
  if (!(stages & ST_ENTRY_QKV) || !w.qkv_ln || !conv_ln_fold_available(c, *w.qkv_ln, x.rows())) stages &= ~ST_ENTRY_LN1;
  return stages;
}

Act st_entry_proj_in(Ctx& c, const StEntryW& w, const Act& x, int stages) {
  const int B = x.B, T = x.H * x.W, C = w.norm.C;
  ConvOpts p0; p0.pad = 0;
  stages = st_entry_effective(c, w, x, stages);
  Act h;
  if (stages & ST_ENTRY_GN) {  // GroupNorm's statistics fold only; proj_in applies the coefficients to its A fragments
    const float* coef = groupnorm_coef_fwd(c, w.norm, x);
    h = alloc_act(c, B, x.H, x.W, C);
    launch_lin_stream_gn(c.st, x.p, x.ld, (int)x.rows(), T, coef, w.proj_in->wfrag, w.proj_in->b, h.p, h.ld);
  } else {
    Act n = groupnorm_fwd(c, w.norm, x, nullptr, false);
    h = conv_fwd(c, *w.proj_in, n, nullptr, p0);  // tokens [B*T][C]
  }
  return h;
}

StEntryOut st_entry_qkv(Ctx& c, const StEntryW& w, const Act& h, int stages) {
  const int B = h.B, T = h.H * h.W, C = w.norm.C;
  ConvOpts p0; p0.pad = 0;
  stages = st_entry_effective(c, w, h, stages);
  CD_CHECK(!w.vbias || (stages & ST_ENTRY_QKV), "transformer entry: a value bias needs the q | k | v launch");
  StEntryOut r;
  r.h = h;
  r.stages = stages & ~ST_ENTRY_GN;
  r.Tpad = round_up(T, 64);
  if (stages & ST_ENTRY_QKV) {
    r.qk = alloc_act(c, B, h.H, h.W, 2 * C);
    r.vt = (bf16_t*)c.arena->alloc((size_t)B * C * r.Tpad * 2);  // T % 256 == 0: no padding columns to clear
    const bool ln = (stages & ST_ENTRY_LN1) != 0;
    Act a = ln ? r.h : layernorm_fwd(c, w.ln1, r.h);
    const ConvW& wq = ln ? *w.qkv_ln : *w.qkv;
    launch_lin_stream_qkv(c.st, a.p, a.ld, (int)a.rows(), T, wq.wfrag, wq.b, r.qk.p, r.vt, r.Tpad, ln, 1e-5f);
    return r;
  }
  Act n1 = layernorm_fwd(c, w.ln1, r.h);
  r.qk = conv_fwd(c, *w.qk1, n1, nullptr, p0);  // [B*T][2C]
  r.vt = (bf16_t*)c.arena->alloc((size_t)B * C * r.Tpad * 2);
  if (r.Tpad != T) HIP_CHECK(hipMemsetAsync(r.vt, 0, (size_t)B * C * r.Tpad * 2, c.st));
  vt_gemm_fwd(c, *w.v1, n1.p, n1.ld, B, T, r.Tpad, r.vt);
  return r;
}

StEntryOut st_entry_fwd(Ctx& c, const StEntryW& w, const Act& x, int stages) {
  const int gn = st_entry_effective(c, w, x, stages) & ST_ENTRY_GN;
  StEntryOut r = st_entry_qkv(c, w, st_entry_proj_in(c, w, x, stages), stages);
  r.stages |= gn;  // (st_entry_qkv sees h, which has x's shape: the same gate)
  return r;
}

Act avgpool2_fwd(Ctx& c, const Act& x) {
  if (x.split) {
    Act y = alloc_act(c, x.B, x.H / 2, x.W / 2, x.C);
    y.split = true; y.ld = 2 * x.C;
    launch_avgpool2_split(c.st, x.p, y.p, x.B, x.H, x.W, x.C, c.overflow);
    return y;
  }
  CD_CHECK(x.ld == x.C, "avgpool: dense input expected");
  Act y = alloc_act(c, x.B, x.H / 2, x.W / 2, x.C);
  if (c.f32) launch_avgpool2_f32(c.st, x.pf(), y.pf(), x.B, x.H, x.W, x.C);
  else launch_avgpool2(c.st, x.p, y.p, x.B, x.H, x.W, x.C);
  return y;
}
Act upsample2_fwd(Ctx& c, const Act& x) {
  CD_CHECK(x.ld == x.C && !x.split, "upsample: dense input expected");
  Act y = alloc_act(c, x.B, x.H * 2, x.W * 2, x.C);
  if (c.f32) launch_upsample2_f32(c.st, x.pf(), y.pf(), x.B, x.H, x.W, x.C);
  else launch_upsample2(c.st, x.p, y.p, x.B, x.H, x.W, x.C);
  return y;
}
Act attention_f32_fwd(Ctx& c, const Act& qk, const Act& v, int H, int D, float scale, const float* obias) {
  CD_CHECK(c.f32 && qk.f32 && v.f32 && !qk.split && !v.split && qk.C == 2 * H * D && v.C == H * D,
           "attention_f32: operands");
  Act o = alloc_act(c, qk.B, qk.H, qk.W, H * D);
  const int T = qk.H * qk.W;
  if (D <= 160 && (D % 4) == 0 && (qk.ld % 4) == 0 && (v.ld % 4) == 0) {
    // round 5: heads up to 160 wide (the improved-DDPM AttentionBlocks: 64) on the fp32 flash kernel of st_f32.hip - fp32
    // matrix instructions instead of one wave per query (3 % of a config-5 step); wider single heads (Ho-DDPM, the KL-f8
    // first stage: d = C) stay on k_attention_f32
    launch_flash_f32(c.st, qk.pf(), qk.ld, (int64_t)T * qk.ld, qk.pf() + H * D, qk.ld, (int64_t)T * qk.ld, v.pf(), v.ld,
                     (int64_t)T * v.ld, o.pf(), o.ld, (int64_t)T * o.ld, qk.B, H, T, T, D, scale * 1.44269504088896340736f, 0,
                     c.overflow, obias);
    return o;
  }
  launch_attention_f32(c.st, qk.pf(), qk.ld, qk.pf() + H * D, qk.ld, v.pf(), v.ld, o.pf(), o.ld, qk.B, H, T, D, scale, obias);
  return o;
}

Act layernorm_fwd(Ctx& c, const LNW& w, const Act& x) {
  CD_CHECK(x.C == w.C, "layernorm: channels");
  if (c.f32) {  // fp32 rows; in the split mode the output is the fp16 pair the next three-term GEMM consumes
    CD_CHECK(x.f32 && !x.split, "layernorm_f32: operand precision");
    Act y = alloc_act(c, x.B, x.H, x.W, x.C);
    if (c.x3) { y.split = true; y.ld = 2 * x.C; }  // same bytes as the fp32 tensor
    launch_layernorm_f32(c.st, x.pf(), x.ld, y.pf(), x.rows(), x.C, w.g, w.b, 1e-5f, c.x3 ? 1 : 0, c.overflow);
    return y;
  }
  Act y = alloc_act(c, x.B, x.H, x.W, x.C);
  launch_layernorm(c.st, x.p, x.ld, y.p, y.ld, (int)x.rows(), x.C, w.g, w.b, 1e-5f);
  return y;
}

Act attention_fwd(Ctx& c, const bf16_t* q, int ldq, const bf16_t* k, int ldk, const bf16_t* v, int ldv, int B,
                  int H, int Tq, int Tk, int D, float scale, int Himg, int Wimg, bool q_log2, int rows) {
  CD_CHECK(!c.f32, "attention: 16-bit kernel called on the fp32 path");
  CD_CHECK(rows <= B, "attention: %d rows of a batch of %d", rows, B);
  Act o = alloc_act(c, B, Himg, Wimg, H * D);
  AttnParams p;
  p.q = q; p.k = k; p.v = v; p.o = o.p;
  p.B = rows >= 0 ? rows : B; p.H = H; p.Tq = Tq; p.Tk = Tk; p.D = D;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = o.ld;
  p.q_bs = (int64_t)Tq * ldq; p.k_bs = (int64_t)Tk * ldk; p.v_bs = (int64_t)Tk * ldv; p.o_bs = (int64_t)Tq * o.ld;
  p.scale = scale; p.q_log2 = q_log2 ? 1 : 0;
  launch_attention(c.st, p);
  return o;
}

Act attention_vt_fwd(Ctx& c, const bf16_t* q, int ldq, const bf16_t* k, int ldk, const bf16_t* vt, int B,
                     int H, int Tq, int Tk, int Tpad, int D, float scale, int Himg, int Wimg, bool q_log2,
                     const float* obias, Act o) {
  CD_CHECK(!c.f32, "attention: 16-bit kernel called on the fp32 path");
  if (!o.p) o = alloc_act(c, B, Himg, Wimg, H * D);
  AttnParams p;
  p.q = q; p.k = k; p.vt = vt; p.o = o.p;
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk; p.D = D;
  p.ldq = ldq; p.ldk = ldk; p.ldo = o.ld;
  p.q_bs = (int64_t)Tq * ldq; p.k_bs = (int64_t)Tk * ldk; p.o_bs = (int64_t)Tq * o.ld;
  p.vt_dpad = D; p.vt_tpad = Tpad;
  p.scale = scale; p.q_log2 = q_log2 ? 1 : 0; p.obias = obias;
  launch_attention(c.st, p);
  return o;
}

Act attention_flash_f32_fwd(Ctx& c, const float* q, int ldq, const float* k, int ldk, int64_t k_bs, const float* v, int ldv,
                            int64_t v_bs, int B, int H, int Tq, int Tk, int D, float scale, int Himg, int Wimg, bool q_log2) {
  CD_CHECK(c.f32, "attention_flash_f32: fp32 path only");
  Act o = alloc_act(c, B, Himg, Wimg, H * D);
  // split mode: the output feeds to_out as fp16 pairs (same bytes as the fp32 tensor; range guard as for the norms)
  launch_flash_f32(c.st, q, ldq, (int64_t)Tq * ldq, k, ldk, k_bs, v, ldv, v_bs, o.pf(), o.ld, (int64_t)Tq * o.ld, B, H, Tq,
                   Tk, D, q_log2 ? 1.0f : scale * 1.44269504088896340736f, c.x3 ? 1 : 0, c.overflow);
  if (c.x3) { o.split = true; o.ld = 2 * o.C; }
  return o;
}

Act geglu_f32_fwd(Ctx& c, const Act& h) {
  CD_CHECK(c.f32 && h.f32 && !h.split && h.ld == h.C && (h.C % 64) == 0, "geglu_f32: operand");
  Act y = alloc_act(c, h.B, h.H, h.W, h.C / 2);
  launch_geglu_f32(c.st, h.pf(), y.pf(), h.rows(), h.C / 2, c.x3 ? 1 : 0, c.overflow);
  if (c.x3) { y.split = true; y.ld = 2 * y.C; }
  return y;
}

Act split_rows_f32_fwd(Ctx& c, const Act& x, const Act* x2) {
  CD_CHECK(c.f32 && c.x3 && x.f32 && !x.split && (!x2 || (x2->f32 && !x2->split && x2->rows() == x.rows())),
           "split_rows_f32: operand");
  const int C = x.C + (x2 ? x2->C : 0);
  Act y = alloc_act(c, x.B, x.H, x.W, C);
  launch_split_rows_f32(c.st, x.pf(), x.ld, x.C, x2 ? x2->pf() : nullptr, x2 ? x2->ld : 4, x2 ? x2->C : 0, y.p, x.rows(),
                        c.overflow);
  y.split = true; y.ld = 2 * C;
  return y;
}


// ------------------------------------------------------------------ blocks shared by the conv nets
GNW make_gn(ParamStore& ps, const std::string& pfx, int C, float eps) {
  GNW g; g.C = C; g.eps = eps;
  g.g = ps.new_vec(C, 1.f); g.b = ps.new_vec(C, 0.f);
  ps.vec(pfx + ".weight", g.g, C);
  ps.vec(pfx + ".bias", g.b, C);
  return g;
}
LNW make_ln(ParamStore& ps, const std::string& pfx, int C) {
  LNW g; g.C = C;
  g.g = ps.new_vec(C, 1.f); g.b = ps.new_vec(C, 0.f);
  ps.vec(pfx + ".weight", g.g, C);
  ps.vec(pfx + ".bias", g.b, C);
  return g;
}
ConvW* make_conv(ParamStore& ps, const std::string& pfx, int N, int Cin, int k, bool bias, bool geglu, int ref_ndim,
                 float wscale) {
  CD_CHECK(!(bias && wscale != 1.f), "a folded weight scale needs the bias scaled too");
  ConvW* c = ps.new_conv(N, Cin, k, k, bias, geglu);
  ps.conv_weight(pfx + ".weight", c, ref_ndim, wscale);
  if (bias) ps.conv_bias(pfx + ".bias", c);
  return c;
}

Act net_input_act(const void* p, int B, int H, int W, int C, bool f32, bool x3) {
  Act x; x.p = (bf16_t*)p; x.B = B; x.H = H; x.W = W; x.C = C; x.ld = C; x.f32 = f32;
  if (x3) { x.split = true; x.ld = 2 * C; }  // the caller hands a split-mode network its input as fp16 pairs
  return x;
}

float* time_emb_fwd(Ctx& c, const TimeEmb& te, const UNetIO& io) {
  const int tB = io.t_shared ? 1 : io.B;
  float* sinu = (float*)c.arena->alloc((size_t)tB * te.dim * 4);
  float* e1 = (float*)c.arena->alloc((size_t)tB * te.hidden * 4);
  float* emb = (float*)c.arena->alloc((size_t)tB * te.hidden * 4);
  float* proj = (float*)c.arena->alloc((size_t)tB * te.proj_total * 4);
  launch_timestep_embedding(c.st, io.tab, io.step, io.t_explicit, sinu, tB, te.dim, te.mode);
  launch_vec_linear(c.st, sinu, te.dim, te.w0, te.b0, e1, te.hidden, tB, te.dim, te.hidden, 0, 1);
  launch_vec_linear(c.st, e1, te.hidden, te.w1, te.b1, emb, te.hidden, tB, te.hidden, te.hidden, 0, 0);
  launch_vec_linear(c.st, emb, te.hidden, te.proj_w, te.proj_b, proj, te.proj_total, tB, te.hidden, te.proj_total, 1, 0);
  return proj;
}

Act res_fwd(Ctx& c, const ResW& r, const Act& x, const Act* x2, const float* proj, int proj_ld, bool t_shared) {
  // output first (it outlives the block's temporaries)
  const int Ho = r.up ? x.H * 2 : (r.down ? x.H / 2 : x.H);
  const int Wo = r.up ? x.W * 2 : (r.down ? x.W / 2 : x.W);
  Act out = alloc_act(c, x.B, Ho, Wo, r.cout, /*with_stats=*/true);
  const int rpv = t_shared ? INT_MAX : Ho * Wo;  // output rows sharing one time-embedding vector
  const size_t mk = c.arena->mark();
  Act h = groupnorm_fwd(c, r.gn1, x, x2, /*silu=*/true);
  Act xs = x;           // skip-path input (identity path needs a single dense tensor)
  const Act* xs2 = x2;
  bool up_in_conv = false;
  if (r.down) {
    CD_CHECK(!x2, "resblock_updown with concat input is not produced by the reference");
    h = avgpool2_fwd(c, h);
    xs = avgpool2_fwd(c, x); xs2 = nullptr;
  } else if (r.up) {
    CD_CHECK(!x2, "resblock_updown with concat input is not produced by the reference");
    up_in_conv = true;
    xs = upsample2_fwd(c, x); xs2 = nullptr;
  }
  CD_CHECK(r.emb_off >= 0 || !r.film, "ResBlock: FiLM without a time-embedding row");
  ConvOpts o1; o1.up = up_in_conv; o1.want_stats = true;
  const float* pr = r.emb_off >= 0 ? proj + r.emb_off : nullptr;
  if (pr && !r.film) { o1.rowvec = pr; o1.rowvec_ld = proj_ld; o1.rows_per_vec = rpv; }
  Act h2 = conv_fwd(c, *r.conv1, h, nullptr, o1);
  Act h3;
  if (r.film) h3 = groupnorm_fwd(c, r.gn2, h2, nullptr, true, pr, t_shared ? 0 : proj_ld);
  else h3 = groupnorm_fwd(c, r.gn2, h2, nullptr, true);
  Act skip;
  if (r.skip) {
    ConvOpts os; os.pad = 0;
    // (Round 4 measured the split form of this projection - its unnormalised input, or the concat of two, first written as
    // fp16 pairs by split_rows_f32_fwd: on config 5 the conversion pass over the 256 x 256 tensors costs more than k_conv_f32
    // saves - 2.93 -> 2.82 images/s same box, profiles/r4_c5r_split_skip_projection_ab.txt - so it stays on the fp32 matrix
    // instructions.)
    skip = conv_fwd(c, *r.skip, xs, xs2, os);
  } else {
    CD_CHECK(!xs2, "identity skip with concat input");
    skip = xs;
  }
  ConvOpts o2; o2.resid = &skip; o2.out = out.p; o2.out_ld = out.ld; o2.out_stats = out.stats_buf;
  conv_fwd(c, *r.conv2, h3, nullptr, o2);
  out.stats = out.stats_buf;
  c.arena->release(mk);
  return out;
}

AtCoreOut at_core(Ctx& c, const ConvW& wv, const float* vbias, const Act& qk, const Act& n, int C, int heads, Act o) {
  const int B = n.B, T = n.H * n.W, D = C / heads;
  AtCoreOut r;
  const int Tpad = round_up(T, 64);
  bf16_t* vt = (bf16_t*)c.arena->alloc((size_t)B * C * Tpad * 2);
  if (Tpad != T) HIP_CHECK(hipMemsetAsync(vt, 0, (size_t)B * C * Tpad * 2, c.st));
  vt_gemm_fwd(c, wv, n.p, n.ld, B, T, Tpad, vt);
  const float scale = 1.0f / sqrtf((float)D);  // w_ * int(c)**(-0.5), model.py:192 (one head: D = C)
  if (!o.p) o = alloc_act(c, B, n.H, n.W, C);
  if (D <= 160) {
    attention_vt_fwd(c, qk.p, qk.ld, qk.p + C, qk.ld, vt, B, heads, T, T, Tpad, D, scale, n.H, n.W, /*q_log2=*/false, vbias, o);
  } else {
    // wide single head (VAE mid block: 4096 tokens x 512 ch): scores materialised once per image,
    // S = QK^T and O = PV on the MFMA GEMM kernel, fp32 row softmax in between
    CD_CHECK(heads == 1, "AttnBlock: heads of %d channels (above 160) are only built for the single-head blocks of the first "
             "stage and the Ho-DDPM U-Net, got %d heads", D, heads);
    CD_CHECK(T % 32 == 0, "AttnBlock: token count %d must be a multiple of 32", T);
    float* S = (float*)c.arena->alloc((size_t)B * T * T * 4);
    bf16_t* P = (bf16_t*)c.arena->alloc((size_t)B * T * T * 2);
    ConvGemmParams g;
    g.src0 = qk.p; g.C0 = C; g.ld0 = qk.ld; g.B = 1; g.Hs = T; g.Ws = 1; g.Hin = T; g.Win = 1;
    g.Hout = T; g.Wout = 1; g.M = T;
    g.wgt = qk.p + C; g.Ktot = C; g.ldw = qk.ld; g.N = T;
    g.nbatch = B; g.a_bs = (int64_t)T * qk.ld; g.w_bs = (int64_t)T * qk.ld; g.o_bs = (int64_t)T * T;
    g.alpha = scale; g.out = S; g.out_ld = T; g.out_f32 = 1; g.zeros = c.zeros;
    launch_conv_gemm(c.st, g);
    launch_softmax_rows(c.st, S, T, P, T, (int64_t)B * T, T);
    ConvGemmParams h;
    h.src0 = P; h.C0 = T; h.ld0 = T; h.B = 1; h.Hs = T; h.Ws = 1; h.Hin = T; h.Win = 1;
    h.Hout = T; h.Wout = 1; h.M = T;
    h.wgt = vt; h.Ktot = T; h.ldw = Tpad; h.N = C;
    h.nbatch = B; h.a_bs = (int64_t)T * T; h.w_bs = (int64_t)C * Tpad; h.o_bs = (int64_t)T * o.ld;
    h.bias = vbias; h.out = o.p; h.out_ld = o.ld; h.zeros = c.zeros;
    launch_conv_gemm(c.st, h);
    r.branch = 1;
  }
  r.o = o; r.vt = vt; r.Tpad = Tpad;
  return r;
}

Act attn_block_fwd(Ctx& c, const AttnW& a, const Act& x) {
  const int C = a.C, D = C / a.heads;
  Act out = alloc_act(c, x.B, x.H, x.W, C, /*with_stats=*/true);
  const size_t mk = c.arena->mark();
  ConvOpts p0; p0.pad = 0;
  Act n = groupnorm_fwd(c, a.norm, x, nullptr, false);
  Act qk = conv_fwd(c, *a.qk, n, nullptr, p0);  // [B*T][2C]
  ConvOpts po; po.pad = 0; po.resid = &x; po.out = out.p; po.out_ld = out.ld;
  if (c.f32) {  // fp32 path: V as ordinary tokens, its bias added to the output (rows of P sum to 1)
    Act v = conv_fwd(c, *a.v, n, nullptr, p0);
    Act o = attention_f32_fwd(c, qk, v, a.heads, D, 1.0f / sqrtf((float)D), a.vbias);
    conv_fwd(c, *a.proj, o, nullptr, po);
  } else {
    Act o = at_core(c, *a.v, a.vbias, qk, n, C, a.heads).o;
    po.out_stats = out.stats_buf;
    conv_fwd(c, *a.proj, o, nullptr, po);
    out.stats = out.stats_buf;
  }
  c.arena->release(mk);
  return out;
}

}  // namespace cd

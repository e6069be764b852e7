// The FID Inception-v3 (evaluation metrics FID / KID): torchvision `Inception3` up to its 2048-d pool3
// features, with the four blocks pytorch-fid and clean-fid replace (FIDInceptionA / C / E_1 / E_2: the branch pools of
// Mixed_5b..7b are 3 x 3 average pools that do not count padding taps, Mixed_7c's is a 3 x 3 max pool). Weights are keyed
// by the names of that network's state_dict (`Conv2d_1a_3x3.conv.weight`, `Mixed_5b.branch1x1.bn.running_var`, ...): a
// pytorch-fid `pt_inception-2015-12-05-*.pth` loads unchanged; `fc.*` is not part of the network.
//
// Every BasicConv2d (conv without bias, BatchNorm eps 1e-3, ReLU) is ONE implicit-GEMM launch (conv_gemm.hip) with the
// BatchNorm folded into its packed weights and bias and ReLU in the epilogue. Every branch writes straight into its channel
// slice of the block's concat buffer (out_ld = the concat width), so concatenation costs nothing. Layers whose output width
// is not a multiple of 32 (80, 48) run with N rounded up to 32: the extra weight rows and bias entries are zero, so the GEMM
// itself writes the zero padding channels their consumer reads. The pools are the bandwidth-bound kernels below: one pass,
// 16-byte channel vectors.
#include "engine.h"

#include <math.h>

namespace cd {

namespace {

constexpr float kBnEps = 1e-3f;  // torchvision BasicConv2d: nn.BatchNorm2d(out_channels, eps=0.001)

int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 65536) g = 65536;
  return (int)(g < 1 ? 1 : g);
}

// 3 x 3 pool over 16-bit NHWC, one thread per (output pixel, 8 channels). MAX: max over the in-image taps; AVG: mean over the
// in-image taps (count_include_pad = False). x: [B][H][W] pixels of stride ldx, y: [B][Ho][Wo] pixels of stride ldy.
template <bool MAX>
__global__ __launch_bounds__(256) void k_pool3x3(const bf16_t* __restrict__ x, int ldx, int B, int H, int W, int C,
                                                 int stride, int pad, bf16_t* __restrict__ y, int ldy, int Ho, int Wo) {
  const int cg = C >> 3;
  const int64_t total = (int64_t)B * Ho * Wo * cg;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % cg);
    const int64_t pix = i / cg;
    const int ox = (int)(pix % Wo);
    const int64_t t = pix / Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = MAX ? -INFINITY : 0.f;
    int n = 0;
    const int iy0 = oy * stride - pad, ix0 = ox * stride - pad;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int iy = iy0 + r;
      if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int ix = ix0 + s;
        if ((unsigned)ix >= (unsigned)W) continue;
        float v[8];
        unpack8(*(const uint4*)(x + ((int64_t)(b * H + iy) * W + ix) * ldx + g * 8), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = MAX ? fmaxf(acc[e], v[e]) : acc[e] + v[e];
        ++n;
      }
    }
    if (!MAX) {
      const float inv = 1.0f / (float)n;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] *= inv;
    }
    *(uint4*)(y + pix * ldy + g * 8) = pack8(acc);
  }
}

// global average pool: x [B][HW] pixels of stride ldx, C channels -> y fp32 [B][C]; one thread per (image, 8 channels)
__global__ __launch_bounds__(256) void k_global_avg(const bf16_t* __restrict__ x, int ldx, int B, int HW, int C,
                                                    float* __restrict__ y) {
  const int cg = C >> 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * cg) return;
  const int b = i / cg, g = i - b * cg;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bf16_t* p = x + (int64_t)b * HW * ldx + g * 8;
  for (int q = 0; q < HW; ++q) {
    float v[8];
    unpack8(*(const uint4*)(p + (int64_t)q * ldx), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += v[e];
  }
  const float inv = 1.0f / (float)HW;
  float4* o = (float4*)(y + (int64_t)b * C + g * 8);
  o[0] = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
  o[1] = make_float4(acc[4] * inv, acc[5] * inv, acc[6] * inv, acc[7] * inv);
}

// BatchNorm fold: raw fp32 conv weight [N][Cin][KH][KW] and the unit's BN vectors -> packed 16-bit rows n < N of
// [Npad][KH][KW][Cpad] (w' = w * gamma / sqrt(var + eps); padding channels zero) and bias[n] = beta - mean * gamma / sqrt(var + eps)
__global__ void k_fold_bn(const float* __restrict__ raw, const float* __restrict__ gamma, const float* __restrict__ beta,
                          const float* __restrict__ mean, const float* __restrict__ var, float eps, int N, int Cin, int KH,
                          int KW, int Cpad, bf16_t* __restrict__ w, float* __restrict__ bias) {
  const int64_t row = (int64_t)KH * KW * Cpad;
  const int64_t total = (int64_t)N * row;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cpad);
    int64_t t = i / Cpad;
    const int s = (int)(t % KW); t /= KW;
    const int r = (int)(t % KH);
    const int n = (int)(t / KH);
    const float sc = gamma[n] / sqrtf(var[n] + eps);
    const float v = c < Cin ? raw[(((int64_t)n * Cin + c) * KH + r) * KW + s] * sc : 0.f;
    w[i] = f2bf(v);
    if (i % row == 0) bias[n] = beta[n] - mean[n] * sc;
  }
}

}  // namespace

void launch_pool3x3(hipStream_t st, const bf16_t* x, int ldx, int B, int H, int W, int C, bool max, int stride, int pad,
                    bf16_t* y, int ldy) {
  CD_CHECK(C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "inception_fid: pool channels");
  const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
  const int64_t n = (int64_t)B * Ho * Wo * (C / 8);
  if (max)
    hipLaunchKernelGGL(k_pool3x3<true>, dim3(grid_for(n)), dim3(256), 0, st, x, ldx, B, H, W, C, stride, pad, y, ldy, Ho, Wo);
  else
    hipLaunchKernelGGL(k_pool3x3<false>, dim3(grid_for(n)), dim3(256), 0, st, x, ldx, B, H, W, C, stride, pad, y, ldy, Ho, Wo);
}

void launch_global_avg(hipStream_t st, const bf16_t* x, int ldx, int B, int HW, int C, float* y) {
  CD_CHECK(C % 8 == 0 && ldx % 8 == 0, "inception_fid: global average pool channels");
  const int n = B * (C / 8);
  hipLaunchKernelGGL(k_global_avg, dim3((n + 255) / 256), dim3(256), 0, st, x, ldx, B, HW, C, y);
}

void launch_fold_bn(hipStream_t st, const float* raw, const float* gamma, const float* beta, const float* mean, const float* var,
                    int N, int Cin, int KH, int KW, int Cpad, bf16_t* w, float* bias) {
  const int64_t n = (int64_t)N * KH * KW * Cpad;
  hipLaunchKernelGGL(k_fold_bn, dim3(grid_for(n)), dim3(256), 0, st, raw, gamma, beta, mean, var, kBnEps, N, Cin, KH, KW, Cpad,
                     w, bias);
}

ConvGemmParams basic_conv_params(const bf16_t* x, int ldx, int B, int H, int W, int Cpad, const bf16_t* wgt, const float* bias,
                                 int N, int KH, int KW, int stride, int pad_t, int pad_l, void* out, int out_ld,
                                 const bf16_t* zeros) {
  ConvGemmParams p;
  p.src0 = x; p.C0 = Cpad; p.ld0 = ldx;
  p.B = B; p.Hs = H; p.Ws = W; p.Hin = H; p.Win = W;
  p.KH = KH; p.KW = KW; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l;
  p.Hout = (H + 2 * pad_t - KH) / stride + 1;
  p.Wout = (W + 2 * pad_l - KW) / stride + 1;
  p.M = B * p.Hout * p.Wout;
  p.wgt = wgt; p.Ktot = KH * KW * Cpad; p.N = round_up(N, 32);
  p.bias = bias; p.act = ACT_RELU;
  p.out = out; p.out_ld = out_ld; p.zeros = zeros;
  return p;
}

namespace {

// one BasicConv2d
struct Unit {
  ConvW* w = nullptr;
  float* raw = nullptr;  // fp32 [N][Cin][KH][KW] as loaded
  float *gamma = nullptr, *beta = nullptr, *mean = nullptr, *var = nullptr;
  int N = 0, Cin = 0, KH = 1, KW = 1, stride = 1, pad_t = 0, pad_l = 0;
};

class InceptionFID : public Net {
 public:
  static constexpr int kRes = 299;

  explicit InceptionFID(const cd_net_desc& d) {
    desc = d;
    CD_CHECK(d.precision == CD_PREC_16, "inception_fid: only the 16-bit precision (CD_PREC_16) is implemented, got %d",
             d.precision);
    CD_CHECK(d.image_size == kRes, "inception_fid: image_size must be %d (got %d)", kRes, d.image_size);
    // stem
    c1a_ = unit("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0);
    c2a_ = unit("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0);
    c2b_ = unit("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1);
    c3b_ = unit("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0);
    c4a_ = unit("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0);
    // Mixed_5b / 5c / 5d (FIDInceptionA)
    const int a_in[3] = {192, 256, 288}, a_pf[3] = {32, 64, 64};
    const char* a_nm[3] = {"Mixed_5b", "Mixed_5c", "Mixed_5d"};
    for (int i = 0; i < 3; ++i) {
      const std::string p = a_nm[i];
      BlockA b;
      b.pf = a_pf[i];
      b.b1 = unit(p + ".branch1x1", a_in[i], 64, 1, 1, 1, 0, 0);
      b.b5_1 = unit(p + ".branch5x5_1", a_in[i], 48, 1, 1, 1, 0, 0);
      b.b5_2 = unit(p + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2);
      b.d1 = unit(p + ".branch3x3dbl_1", a_in[i], 64, 1, 1, 1, 0, 0);
      b.d2 = unit(p + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
      b.d3 = unit(p + ".branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1);
      b.bp = unit(p + ".branch_pool", a_in[i], a_pf[i], 1, 1, 1, 0, 0);
      a_.push_back(b);
    }
    // Mixed_6a (InceptionB)
    b_.b3 = unit("Mixed_6a.branch3x3", 288, 384, 3, 3, 2, 0, 0);
    b_.d1 = unit("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 1, 0, 0);
    b_.d2 = unit("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
    b_.d3 = unit("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0);
    // Mixed_6b..6e (FIDInceptionC)
    const int c7s[4] = {128, 160, 160, 192};
    const char* c_nm[4] = {"Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"};
    for (int i = 0; i < 4; ++i) {
      const std::string p = c_nm[i];
      const int c7 = c7s[i];
      BlockC b;
      b.b1 = unit(p + ".branch1x1", 768, 192, 1, 1, 1, 0, 0);
      b.s1 = unit(p + ".branch7x7_1", 768, c7, 1, 1, 1, 0, 0);
      b.s2 = unit(p + ".branch7x7_2", c7, c7, 1, 7, 1, 0, 3);
      b.s3 = unit(p + ".branch7x7_3", c7, 192, 7, 1, 1, 3, 0);
      b.d1 = unit(p + ".branch7x7dbl_1", 768, c7, 1, 1, 1, 0, 0);
      b.d2 = unit(p + ".branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0);
      b.d3 = unit(p + ".branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3);
      b.d4 = unit(p + ".branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0);
      b.d5 = unit(p + ".branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3);
      b.bp = unit(p + ".branch_pool", 768, 192, 1, 1, 1, 0, 0);
      c_.push_back(b);
    }
    // Mixed_7a (InceptionD)
    d_.t1 = unit("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 1, 0, 0);
    d_.t2 = unit("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2, 0, 0);
    d_.s1 = unit("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1, 1, 0, 0);
    d_.s2 = unit("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3);
    d_.s3 = unit("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0);
    d_.s4 = unit("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0);
    // Mixed_7b (FIDInceptionE_1, average branch pool) and Mixed_7c (FIDInceptionE_2, max branch pool)
    const int e_in[2] = {1280, 2048};
    const char* e_nm[2] = {"Mixed_7b", "Mixed_7c"};
    for (int i = 0; i < 2; ++i) {
      const std::string p = e_nm[i];
      BlockE b;
      b.max_pool = i == 1;
      b.b1 = unit(p + ".branch1x1", e_in[i], 320, 1, 1, 1, 0, 0);
      b.t1 = unit(p + ".branch3x3_1", e_in[i], 384, 1, 1, 1, 0, 0);
      b.t2a = unit(p + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1);
      b.t2b = unit(p + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0);
      b.d1 = unit(p + ".branch3x3dbl_1", e_in[i], 448, 1, 1, 1, 0, 0);
      b.d2 = unit(p + ".branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1);
      b.d3a = unit(p + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1);
      b.d3b = unit(p + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0);
      b.bp = unit(p + ".branch_pool", e_in[i], 192, 1, 1, 1, 0, 0);
      e_.push_back(b);
    }
  }
  int kind() const override { return CD_NET_INCEPTION_FID; }

  // img fp32 NCHW [B][3][299][299] (normalised); stop_block < 0: pool3 fp32 [B][2048]; else the output of block list entry
  // stop_block as fp32 NCHW (include/cyclediff.h cd_inception_features)
  void features(Ctx& c, const float* img, int B, int stop_block, float* out) {
    CD_CHECK(B > 0 && stop_block >= -1 && stop_block < kNumBlocks, "inception_fid: bad batch %d / stop_block %d", B, stop_block);
    fold_if_needed(c);
    const size_t mk = c.arena->mark();
    int blk = 0;
    Act x = alloc_act(c, B, kRes, kRes, 32);  // 3 channels, zero padded to 32
    launch_nchw_to_nhwc(c.st, img, x.p, B, 3, kRes * kRes, 32, 1.f, 0.f, 0);
    x.C = 3;
    auto emit = [&](const Act& a) {  // true: this was the requested block (its fp32 NCHW copy is written)
      if (blk++ != stop_block) return false;
      launch_nhwc_to_nchw(c.st, a.p, 0, a.ld, out, a.B, a.C, a.H * a.W, 1.f, 0.f);
      return true;
    };
    // stem: 299 -> 149 -> 147 -> 147 -> 73 -> 73 -> 71 -> 35
    Act h = conv_new(c, c1a_, x);
    if (emit(h)) return done(c, mk);
    h = conv_new(c, c2a_, h);
    if (emit(h)) return done(c, mk);
    h = conv_new(c, c2b_, h);
    if (emit(h)) return done(c, mk);
    h = pool_new(c, h, true, 2, 0);
    if (emit(h)) return done(c, mk);
    h = conv_new(c, c3b_, h);
    if (emit(h)) return done(c, mk);
    h = conv_new(c, c4a_, h);
    if (emit(h)) return done(c, mk);
    h = pool_new(c, h, true, 2, 0);
    if (emit(h)) return done(c, mk);
    for (const BlockA& b : a_) {
      h = block_a(c, b, h);
      if (emit(h)) return done(c, mk);
    }
    h = block_b(c, h);
    if (emit(h)) return done(c, mk);
    for (const BlockC& b : c_) {
      h = block_c(c, b, h);
      if (emit(h)) return done(c, mk);
    }
    h = block_d(c, h);
    if (emit(h)) return done(c, mk);
    for (const BlockE& b : e_) {
      h = block_e(c, b, h);
      if (emit(h)) return done(c, mk);
    }
    CD_CHECK(h.C == 2048 && h.H == 8 && h.W == 8 && (h.ld % 8) == 0, "inception_fid: pool3 input shape");
    launch_global_avg(c.st, h.p, h.ld, B, 64, 2048, out);
    done(c, mk);
  }
  // stem convs and pools (7), Mixed_5b..5d (3), 6a, 6b..6e (4), 7a, 7b, 7c
  static constexpr int kNumBlocks = 18;

 private:
  struct BlockA { Unit b1, b5_1, b5_2, d1, d2, d3, bp; int pf = 0; };
  struct BlockB { Unit b3, d1, d2, d3; };
  struct BlockC { Unit b1, s1, s2, s3, d1, d2, d3, d4, d5, bp; };
  struct BlockD { Unit t1, t2, s1, s2, s3, s4; };
  struct BlockE { Unit b1, t1, t2a, t2b, d1, d2, d3a, d3b, bp; bool max_pool = false; };

  void done(Ctx& c, size_t mk) { c.arena->release(mk); }

  Unit unit(const std::string& name, int Cin, int N, int KH, int KW, int stride, int pad_t, int pad_l) {
    Unit u;
    u.N = N; u.Cin = Cin; u.KH = KH; u.KW = KW; u.stride = stride; u.pad_t = pad_t; u.pad_l = pad_l;
    u.w = params.new_conv(N, Cin, KH, KW, true);
    u.raw = params.new_vec(N * Cin * KH * KW);
    ParamDecl& d = params.declare(name + ".conv.weight", {N, Cin, KH, KW});
    PackTarget t;
    t.kind = PackTarget::MATRIX_F32; t.fdst = u.raw; t.dst_off = 0; t.rows = N; t.K = Cin * KH * KW;
    t.src_base = 0; t.grp = N; t.grp_stride = 0;
    d.targets.push_back(t);
    u.gamma = params.new_vec(N, 1.f);
    u.beta = params.new_vec(N);
    u.mean = params.new_vec(N);
    u.var = params.new_vec(N, 1.f);
    params.vec(name + ".bn.weight", u.gamma, N);
    params.vec(name + ".bn.bias", u.beta, N);
    params.vec(name + ".bn.running_mean", u.mean, N);
    params.vec(name + ".bn.running_var", u.var, N);
    units_.push_back(u);
    return u;
  }

  // BatchNorm folded into the packed weights once per weight version (every cd_net_load_param bumps it)
  void fold_if_needed(Ctx& c) {
    if (folded_version_ == params.version) return;
    std::string first;
    const int miss = params.missing(&first);
    CD_CHECK(miss == 0, "inception_fid: %d parameters not loaded (first: %s)", miss, first.c_str());
    for (const Unit& u : units_)
      launch_fold_bn(c.st, u.raw, u.gamma, u.beta, u.mean, u.var, u.N, u.Cin, u.KH, u.KW, u.w->Cpad, u.w->w, u.w->b);
    folded_version_ = params.version;
  }

  // conv + folded BN + ReLU into `out` (pixel stride out_ld); N rounded up to 32 (zero rows: zero padding channels)
  Act conv(Ctx& c, const Unit& u, const Act& x, bf16_t* out, int out_ld) {
    const int Cpad = u.w->Cpad, Nrun = round_up(u.N, 32);
    CD_CHECK(x.C == u.Cin && x.ld >= Cpad && out_ld >= Nrun, "inception_fid: conv operand shapes (C %d / Cin %d)", x.C, u.Cin);
    const ConvGemmParams p = basic_conv_params(x.p, x.ld, x.B, x.H, x.W, Cpad, u.w->w, u.w->b, u.N, u.KH, u.KW, u.stride, u.pad_t,
                                               u.pad_l, out, out_ld, c.zeros);
    launch_conv_gemm(c.st, p);
    Act y; y.p = out; y.B = x.B; y.H = p.Hout; y.W = p.Wout; y.C = u.N; y.ld = out_ld;
    return y;
  }
  Act conv_new(Ctx& c, const Unit& u, const Act& x) {
    const int Ho = (x.H + 2 * u.pad_t - u.KH) / u.stride + 1, Wo = (x.W + 2 * u.pad_l - u.KW) / u.stride + 1;
    Act y = alloc_act(c, x.B, Ho, Wo, round_up(u.N, 32));
    return conv(c, u, x, y.p, y.ld);
  }
  Act pool(Ctx& c, const Act& x, bool max, int stride, int pad, bf16_t* out, int out_ld) {
    const int Ho = (x.H + 2 * pad - 3) / stride + 1, Wo = (x.W + 2 * pad - 3) / stride + 1;
    launch_pool3x3(c.st, x.p, x.ld, x.B, x.H, x.W, x.C, max, stride, pad, out, out_ld);
    Act y; y.p = out; y.B = x.B; y.H = Ho; y.W = Wo; y.C = x.C; y.ld = out_ld;
    return y;
  }
  Act pool_new(Ctx& c, const Act& x, bool max, int stride, int pad) {
    Act y = alloc_act(c, x.B, (x.H + 2 * pad - 3) / stride + 1, (x.W + 2 * pad - 3) / stride + 1, x.C);
    return pool(c, x, max, stride, pad, y.p, y.ld);
  }
  // the block's concat buffer; temporaries of the block are released when it returns
  static Act slice(const Act& y, int off, int C) { Act s = y; s.p = y.p + off; s.C = C; return s; }

  Act block_a(Ctx& c, const BlockA& b, const Act& x) {
    const int Ct = 224 + b.pf;
    Act y = alloc_act(c, x.B, x.H, x.W, Ct);
    const size_t mk = c.arena->mark();
    conv(c, b.b1, x, y.p, Ct);
    conv(c, b.b5_2, conv_new(c, b.b5_1, x), y.p + 64, Ct);
    conv(c, b.d3, conv_new(c, b.d2, conv_new(c, b.d1, x)), y.p + 128, Ct);
    conv(c, b.bp, pool_new(c, x, false, 1, 1), y.p + 224, Ct);
    c.arena->release(mk);
    return y;
  }
  Act block_b(Ctx& c, const Act& x) {
    const int Ho = (x.H - 3) / 2 + 1, Wo = (x.W - 3) / 2 + 1, Ct = 384 + 96 + x.C;
    Act y = alloc_act(c, x.B, Ho, Wo, Ct);
    const size_t mk = c.arena->mark();
    conv(c, b_.b3, x, y.p, Ct);
    conv(c, b_.d3, conv_new(c, b_.d2, conv_new(c, b_.d1, x)), y.p + 384, Ct);
    pool(c, x, true, 2, 0, y.p + 480, Ct);
    c.arena->release(mk);
    return y;
  }
  Act block_c(Ctx& c, const BlockC& b, const Act& x) {
    const int Ct = 768;
    Act y = alloc_act(c, x.B, x.H, x.W, Ct);
    const size_t mk = c.arena->mark();
    conv(c, b.b1, x, y.p, Ct);
    conv(c, b.s3, conv_new(c, b.s2, conv_new(c, b.s1, x)), y.p + 192, Ct);
    Act t = conv_new(c, b.d3, conv_new(c, b.d2, conv_new(c, b.d1, x)));
    conv(c, b.d5, conv_new(c, b.d4, t), y.p + 384, Ct);
    conv(c, b.bp, pool_new(c, x, false, 1, 1), y.p + 576, Ct);
    c.arena->release(mk);
    return y;
  }
  Act block_d(Ctx& c, const Act& x) {
    const int Ho = (x.H - 3) / 2 + 1, Wo = (x.W - 3) / 2 + 1, Ct = 320 + 192 + x.C;
    Act y = alloc_act(c, x.B, Ho, Wo, Ct);
    const size_t mk = c.arena->mark();
    conv(c, d_.t2, conv_new(c, d_.t1, x), y.p, Ct);
    Act t = conv_new(c, d_.s3, conv_new(c, d_.s2, conv_new(c, d_.s1, x)));
    conv(c, d_.s4, t, y.p + 320, Ct);
    pool(c, x, true, 2, 0, y.p + 512, Ct);
    c.arena->release(mk);
    return y;
  }
  Act block_e(Ctx& c, const BlockE& b, const Act& x) {
    const int Ct = 2048;
    Act y = alloc_act(c, x.B, x.H, x.W, Ct);
    const size_t mk = c.arena->mark();
    conv(c, b.b1, x, y.p, Ct);
    Act t = conv_new(c, b.t1, x);
    conv(c, b.t2a, t, y.p + 320, Ct);
    conv(c, b.t2b, t, y.p + 704, Ct);
    Act d = conv_new(c, b.d2, conv_new(c, b.d1, x));
    conv(c, b.d3a, d, y.p + 1088, Ct);
    conv(c, b.d3b, d, y.p + 1472, Ct);
    conv(c, b.bp, pool_new(c, x, b.max_pool, 1, 1), y.p + 1856, Ct);
    c.arena->release(mk);
    return y;
  }

  Unit c1a_, c2a_, c2b_, c3b_, c4a_;
  std::vector<BlockA> a_;
  BlockB b_;
  std::vector<BlockC> c_;
  BlockD d_;
  std::vector<BlockE> e_;
  std::vector<Unit> units_;
  int folded_version_ = -1;
};

}  // namespace

std::unique_ptr<Net> make_inception_fid(const cd_net_desc& d) { return std::unique_ptr<Net>(new InceptionFID(d)); }

void inception_fid_features(Net* n, Ctx& c, const float* img, int B, int stop_block, float* out) {
  CD_CHECK(n && n->kind() == CD_NET_INCEPTION_FID, "net is not an Inception-v3 (CD_NET_INCEPTION_FID)");
  static_cast<InceptionFID*>(n)->features(c, img, B, stop_block, out);
}

}  // namespace cd

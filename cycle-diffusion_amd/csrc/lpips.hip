// LPIPS v0.1 (the perceptual distance of Zhang et al. 2018 as the `lpips` package computes it) on the
// AlexNet and VGG16 `features` stacks of torchvision. Weights are keyed `features.N.weight|bias` (N = the torchvision
// `features` index of the conv) and `lin{l}.weight` ([1, C_l, 1, 1], the 1 x 1 `lin` layer of tap l, no bias).
//
// Forward: [x0 | x1] run as ONE batch of 2 B images. The scaling layer is a kernel of its own (fp32 NCHW -> 16-bit NHWC of
// row stride 32, (x - shift) / scale per channel, channels 3..31 zero) and is NOT folded into the first conv: the reference
// zero-pads after scaling, a folded bias would see the shift on the border taps. Every conv + bias + ReLU is one implicit-GEMM
// launch (conv_gemm.hip; every width is a multiple of 32), the 3 x 3 stride-2 pools of AlexNet are launch_pool3x3, the 2 x 2
// stride-2 pools of VGG16 the kernel below. Each tap feeds k_lpips_layer with rows [0, B) against rows [B, 2 B).
#include "engine.h"

#include <math.h>

namespace cd {

namespace {

int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 65536) g = 65536;
  return (int)(g < 1 ? 1 : g);
}

// the package's ScalingLayer constants
constexpr float kShift[3] = {-.030f, -.088f, -.188f};
constexpr float kScale[3] = {.458f, .448f, .450f};

// fp32 NCHW [B][3][HW] -> 16-bit NHWC [B][HW][32]: channel c < 3 = (x - shift[c]) / scale[c], channels 3..31 zero.
// One thread per pixel: three coalesced plane reads, one 64-byte row written as four 16-byte vectors.
__global__ __launch_bounds__(256) void k_lpips_input(const float* __restrict__ x, bf16_t* __restrict__ y, int B, int HW) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW, q = i - b * HW;
    const float* p = x + b * 3 * HW + q;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    v[0] = (p[0] - kShift[0]) / kScale[0];
    v[1] = (p[HW] - kShift[1]) / kScale[1];
    v[2] = (p[2 * (int64_t)HW] - kShift[2]) / kScale[2];
    uint4* o = (uint4*)(y + i * 32);
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    o[0] = pack8(v);
    o[1] = z; o[2] = z; o[3] = z;
  }
}

// 2 x 2 stride-2 max pool (floor of odd sizes) over 16-bit NHWC, one thread per (output pixel, 8 channels).
// x: [B][H][W] pixels of stride ldx, y: [B][H / 2][W / 2] pixels of stride ldy.
__global__ __launch_bounds__(256) void k_pool2x2(const bf16_t* __restrict__ x, int ldx, int B, int H, int W, int C,
                                                 bf16_t* __restrict__ y, int ldy, int Ho, int Wo) {
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
    for (int e = 0; e < 8; ++e) acc[e] = -INFINITY;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[8];
        unpack8(*(const uint4*)(x + ((int64_t)(b * H + 2 * oy + r) * W + 2 * ox + s) * ldx + g * 8), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaxf(acc[e], v[e]);
      }
    }
    *(uint4*)(y + pix * ldy + g * 8) = pack8(acc);
  }
}

// Sum over the LP lanes of a group (LP a power of two <= 64, groups aligned within the wave), result in every lane
template <int LP>
__device__ inline float group_allsum(float v) {
#pragma unroll
  for (int m = LP / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// a / n to within an ulp from the one reciprocal r = 1 / n of the group: one Newton correction of the quotient
__device__ inline float div_refined(float a, float n, float r) {
  const float q = a * r;
  return __builtin_fmaf(__builtin_fmaf(-q, n, a), r, q);
}

constexpr int kLpThreads = 256;
constexpr int kLpIters = 8;  // pixels per group and workgroup
// pixels of one image a workgroup owns: a function of C alone, so the split of an image depends on HW and C, never on B
inline int lp_lanes(int C) { int lp = 8; while (lp * 8 < C) lp *= 2; return lp; }
inline int lp_pixels_per_wg(int C) { return (kLpThreads / lp_lanes(C)) * kLpIters; }

// One LPIPS tap: f0, f1 16-bit [B][HW] pixels of stride ld, C channels, w fp32 [C] ->
//   part[b][chunk] = sum over the chunk's pixels of sum_c w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2
// A pixel is owned by LP = next_pow2(C / 8) lanes (surplus lanes idle); each lane loads 16 bytes of each map once and keeps
// them in registers for both steps: the squared norms (group reduction), then the weighted squared difference of the
// normalised vectors (second group reduction). The expanded one-pass form cancels when the maps are close and is not used.
// No atomics: blockIdx.y = image, blockIdx.x = chunk of kLpIters * (256 / LP) pixels; the groups' sums meet in LDS and lane 0
// adds them in index order.
template <int LP>
__global__ __launch_bounds__(kLpThreads) void k_lpips_layer(const bf16_t* __restrict__ f0, const bf16_t* __restrict__ f1, int ld,
                                                            int HW, int C, const float* __restrict__ w,
                                                            float* __restrict__ part) {
  constexpr int G = kLpThreads / LP;  // groups (pixels in flight) per workgroup
  __shared__ float s_sum[G];
  const int grp = threadIdx.x / LP, lane = threadIdx.x % LP;
  const int b = blockIdx.y;
  const bool live = lane * 8 < C;
  float wv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float4 w0 = *(const float4*)(w + lane * 8), w1 = *(const float4*)(w + lane * 8 + 4);
    wv[0] = w0.x; wv[1] = w0.y; wv[2] = w0.z; wv[3] = w0.w;
    wv[4] = w1.x; wv[5] = w1.y; wv[6] = w1.z; wv[7] = w1.w;
  }
  const int pix0 = blockIdx.x * (G * kLpIters);
  float acc = 0.f;
#pragma unroll 2
  for (int it = 0; it < kLpIters; ++it) {
    const int pix = pix0 + it * G + grp;
    float a[8], c[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] = 0.f; c[e] = 0.f; }
    if (live && pix < HW) {
      const int64_t off = ((int64_t)b * HW + pix) * ld + lane * 8;
      unpack8(*(const uint4*)(f0 + off), a);
      unpack8(*(const uint4*)(f1 + off), c);
    }
    float sa = 0.f, sc = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { sa = __builtin_fmaf(a[e], a[e], sa); sc = __builtin_fmaf(c[e], c[e], sc); }
    sa = group_allsum<LP>(sa);
    sc = group_allsum<LP>(sc);
    const float na = sqrtf(sa) + 1e-10f, nc = sqrtf(sc) + 1e-10f;
    const float ra = 1.0f / na, rc = 1.0f / nc;
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = div_refined(a[e], na, ra) - div_refined(c[e], nc, rc);
      d = __builtin_fmaf(wv[e] * t, t, d);
    }
    acc += group_allsum<LP>(d);  // dead pixels and idle lanes add exactly 0
  }
  if (lane == 0) s_sum[grp] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) s += s_sum[g];
    part[(int64_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// d[b] = (sum of part[b][0 .. n) in index order, in double) / HW; per_layer[b][5] entry `layer` when asked; out[b] = d[b] for
// the first tap, out[b] += d[b] for the later ones (tap order: the launches are stream-ordered)
__global__ void k_lpips_finish(const float* __restrict__ part, int n, int B, float inv_hw, float* __restrict__ per_layer,
                               int layer, int accumulate, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += (double)part[(int64_t)b * n + i];
  const float v = (float)(s * (double)inv_hw);
  if (per_layer) per_layer[b * 5 + layer] = v;
  out[b] = accumulate ? out[b] + v : v;
}

}  // namespace

void launch_lpips_input(hipStream_t st, const float* x, bf16_t* y, int B, int HW) {
  hipLaunchKernelGGL(k_lpips_input, dim3(grid_for((int64_t)B * HW)), dim3(256), 0, st, x, y, B, HW);
}

void launch_pool2x2(hipStream_t st, const bf16_t* x, int ldx, int B, int H, int W, int C, bf16_t* y, int ldy) {
  CD_CHECK(C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "lpips: pool channels");
  CD_CHECK(H >= 2 && W >= 2, "lpips: 2 x 2 pool of a %d x %d image", H, W);
  const int Ho = H / 2, Wo = W / 2;
  const int64_t n = (int64_t)B * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(k_pool2x2, dim3(grid_for(n)), dim3(256), 0, st, x, ldx, B, H, W, C, y, ldy, Ho, Wo);
}

int lpips_layer_chunks(int HW, int C) { return ceil_div(HW, lp_pixels_per_wg(C)); }

void launch_lpips_layer(hipStream_t st, const bf16_t* f0, const bf16_t* f1, int ld, int B, int HW, int C, const float* w,
                        float* part, float* per_layer, int layer, bool accumulate, float* out) {
  CD_CHECK(C > 0 && C % 8 == 0, "lpips_layer: C = %d is not a multiple of 8", C);
  CD_CHECK(C <= 512, "lpips_layer: C = %d exceeds 512", C);
  CD_CHECK(ld % 8 == 0 && ld >= C, "lpips_layer: the pixel stride %d is not a multiple of 8 elements (or below C)", ld);
  CD_CHECK(B > 0 && B <= 65535 && HW > 0 && layer >= 0 && layer < 5, "lpips_layer: bad batch %d / pixels %d / layer %d", B, HW,
           layer);
  CD_CHECK(((uintptr_t)f0 & 15) == 0 && ((uintptr_t)f1 & 15) == 0 && ((uintptr_t)w & 15) == 0, "lpips_layer: 16-B alignment");
  const int n = lpips_layer_chunks(HW, C);
  const dim3 grid(n, B), block(kLpThreads);
  switch (lp_lanes(C)) {
    case 8: hipLaunchKernelGGL(k_lpips_layer<8>, grid, block, 0, st, f0, f1, ld, HW, C, w, part); break;
    case 16: hipLaunchKernelGGL(k_lpips_layer<16>, grid, block, 0, st, f0, f1, ld, HW, C, w, part); break;
    case 32: hipLaunchKernelGGL(k_lpips_layer<32>, grid, block, 0, st, f0, f1, ld, HW, C, w, part); break;
    default: hipLaunchKernelGGL(k_lpips_layer<64>, grid, block, 0, st, f0, f1, ld, HW, C, w, part); break;
  }
  hipLaunchKernelGGL(k_lpips_finish, dim3(ceil_div(B, 64)), dim3(64), 0, st, part, n, B, 1.0f / (float)HW, per_layer, layer,
                     accumulate ? 1 : 0, out);
}

namespace {

struct LpConv {
  ConvW* w = nullptr;
  int Cin = 0, N = 0, k = 3, stride = 1, pad = 1;
  int pool = 0;   // pool ahead of this conv: 0 none, 2 = 2 x 2 stride 2, 3 = 3 x 3 stride 2
  int tap = -1;   // its ReLU output is tap `tap`
};

class Lpips : public Net {
 public:
  explicit Lpips(const cd_net_desc& d) {
    desc = d;
    CD_CHECK(d.precision == CD_PREC_16, "lpips: only the 16-bit precision (CD_PREC_16) is implemented, got %d", d.precision);
    CD_CHECK(d.num_res_blocks == 5 || d.num_res_blocks == 13,
             "lpips: num_res_blocks selects the backbone, 5 = AlexNet or 13 = VGG16 (got %d)", d.num_res_blocks);
    alex_ = d.num_res_blocks == 5;
    if (alex_) {
      add(0, 3, 64, 11, 4, 2, 0, 0);
      add(3, 64, 192, 5, 1, 2, 3, 1);
      add(6, 192, 384, 3, 1, 1, 3, 2);
      add(8, 384, 256, 3, 1, 1, 0, 3);
      add(10, 256, 256, 3, 1, 1, 0, 4);
    } else {
      const int idx[13] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};
      const int width[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
      int cin = 3, tap = 0;
      for (int i = 0; i < 13; ++i) {
        const bool pool = idx[i] == 5 || idx[i] == 10 || idx[i] == 17 || idx[i] == 24;
        const bool is_tap = idx[i] == 2 || idx[i] == 7 || idx[i] == 14 || idx[i] == 21 || idx[i] == 28;
        add(idx[i], cin, width[i], 3, 1, 1, pool ? 2 : 0, is_tap ? tap++ : -1);
        cin = width[i];
      }
    }
    for (const LpConv& l : convs_) {
      if (l.tap < 0) continue;
      lin_[l.tap] = params.new_vec(l.N);
      ParamDecl& pd = params.declare("lin" + std::to_string(l.tap) + ".weight", {1, l.N, 1, 1});
      PackTarget t;
      t.kind = PackTarget::MATRIX_F32; t.fdst = lin_[l.tap]; t.dst_off = 0; t.rows = 1; t.K = l.N;
      t.src_base = 0; t.grp = 1; t.grp_stride = 0;
      pd.targets.push_back(t);
    }
  }
  int kind() const override { return CD_NET_LPIPS; }
  int min_size() const { return alex_ ? 31 : 16; }

  // img0 (and img1, or null in tap mode) fp32 NCHW [B][3][H][W] in [-1, 1].
  // tap < 0: out [B] = the distance, per_layer [B][5] or null; tap 0..4 (img1 null): out = that tap of img0 as fp32 NCHW
  void forward(Ctx& c, const float* img0, const float* img1, int B, int H, int W, int tap, float* per_layer, float* out) {
    CD_CHECK(B >= 1, "lpips: the batch must hold at least one image (got %d)", B);
    CD_CHECK(H >= min_size() && W >= min_size(), "lpips: a %d x %d image leaves a tap of the %s backbone empty, the minimum size is %d",
             H, W, alex_ ? "alex" : "vgg", min_size());
    CD_CHECK((img1 != nullptr) == (tap < 0) && tap < 5, "lpips: bad tap %d", tap);
    std::string first;
    const int miss = params.missing(&first);
    CD_CHECK(miss == 0, "lpips: %d parameters not loaded (first: %s)", miss, first.c_str());
    const int n = img1 ? 2 * B : B;
    CD_CHECK((int64_t)n * H * W < (1ll << 31), "lpips: %d images of %d x %d exceed the row index range", n, H, W);
    const size_t mk0 = c.arena->mark();
    Act x = alloc_act(c, n, H, W, 32);
    launch_lpips_input(c.st, img0, x.p, B, H * W);
    if (img1) launch_lpips_input(c.st, img1, x.p + (int64_t)B * H * W * 32, B, H * W);
    x.C = 3;
    Act cur = x;
    // a stage = the convs up to and including a tap. Where a pool follows, its output is allocated ahead of the stage and the
    // stage's own buffers are released behind it, so the arena holds the pooled inputs and one stage of conv outputs at a time
    size_t i = 0;
    while (i < convs_.size()) {
      size_t e = i;
      while (convs_[e].tap < 0) ++e;  // the stage is convs_[i .. e]
      const bool pool_next = e + 1 < convs_.size() && convs_[e + 1].pool != 0;
      int h = cur.H, wd = cur.W;  // a pooled stage input is already `cur`
      for (size_t j = i; j <= e; ++j) {
        h = (h + 2 * convs_[j].pad - convs_[j].k) / convs_[j].stride + 1;
        wd = (wd + 2 * convs_[j].pad - convs_[j].k) / convs_[j].stride + 1;
      }
      Act nxt;
      if (pool_next) {
        int ph = h, pw = wd;
        pooled(convs_[e + 1].pool, &ph, &pw);
        nxt = alloc_act(c, n, ph, pw, convs_[e].N);
      }
      const size_t mk = c.arena->mark();
      for (size_t j = i; j <= e; ++j) cur = conv_new(c, convs_[j], cur);
      CD_CHECK(cur.H == h && cur.W == wd && h > 0 && wd > 0, "lpips: stage geometry");
      const int t = convs_[e].tap;
      if (tap < 0) {
        const int HW = cur.H * cur.W;
        float* part = (float*)c.arena->alloc((size_t)B * lpips_layer_chunks(HW, cur.C) * sizeof(float));
        launch_lpips_layer(c.st, cur.p, cur.p + (int64_t)B * HW * cur.ld, cur.ld, B, HW, cur.C, lin_[t], part, per_layer, t, t > 0,
                           out);
      } else if (t == tap) {
        launch_nhwc_to_nchw(c.st, cur.p, 0, cur.ld, out, cur.B, cur.C, cur.H * cur.W, 1.f, 0.f);
        break;
      }
      if (pool_next) {
        if (convs_[e + 1].pool == 2) launch_pool2x2(c.st, cur.p, cur.ld, n, cur.H, cur.W, cur.C, nxt.p, nxt.ld);
        else launch_pool3x3(c.st, cur.p, cur.ld, n, cur.H, cur.W, cur.C, true, 2, 0, nxt.p, nxt.ld);
        c.arena->release(mk);
        cur = nxt;
      }
      i = e + 1;
    }
    c.arena->release(mk0);
  }

 private:
  static void pooled(int kind, int* h, int* w) {
    if (kind == 2) { *h /= 2; *w /= 2; }
    else { *h = (*h - 3) / 2 + 1; *w = (*w - 3) / 2 + 1; }
  }
  void add(int idx, int Cin, int N, int k, int stride, int pad, int pool, int tap) {
    LpConv l;
    l.Cin = Cin; l.N = N; l.k = k; l.stride = stride; l.pad = pad; l.pool = pool; l.tap = tap;
    l.w = make_conv(params, "features." + std::to_string(idx), N, Cin, k);
    convs_.push_back(l);
  }
  // conv + bias + ReLU: one implicit-GEMM launch, Cin padded to 32 by the packed weights' zero columns
  Act conv_new(Ctx& c, const LpConv& l, const Act& x) {
    const int Cpad = l.w->Cpad;
    CD_CHECK(x.C == l.Cin && x.ld >= Cpad && l.N % 32 == 0, "lpips: conv operand shapes (C %d / Cin %d)", x.C, l.Cin);
    const Act& in = x;
    const int Ho = (in.H + 2 * l.pad - l.k) / l.stride + 1, Wo = (in.W + 2 * l.pad - l.k) / l.stride + 1;
    Act y = alloc_act(c, in.B, Ho, Wo, l.N);
    const ConvGemmParams p = basic_conv_params(in.p, in.ld, in.B, in.H, in.W, Cpad, l.w->w, l.w->b, l.N, l.k, l.k, l.stride, l.pad,
                                               l.pad, y.p, y.ld, c.zeros);
    launch_conv_gemm(c.st, p);
    return y;
  }

  bool alex_ = true;
  std::vector<LpConv> convs_;
  float* lin_[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

Lpips* as_lpips(Net* n) {
  CD_CHECK(n && n->kind() == CD_NET_LPIPS, "net is not an LPIPS network (CD_NET_LPIPS)");
  return static_cast<Lpips*>(n);
}

}  // namespace

std::unique_ptr<Net> make_lpips(const cd_net_desc& d) { return std::unique_ptr<Net>(new Lpips(d)); }

void lpips_distance(Net* n, Ctx& c, const float* img0, const float* img1, int B, int H, int W, float* per_layer, float* out) {
  as_lpips(n)->forward(c, img0, img1, B, H, W, -1, per_layer, out);
}

void lpips_tap(Net* n, Ctx& c, const float* img, int B, int H, int W, int tap, float* out) {
  CD_CHECK(tap >= 0 && tap < 5, "lpips: tap %d outside 0..4", tap);
  as_lpips(n)->forward(c, img, nullptr, B, H, W, tap, nullptr, out);
}

}  // namespace cd

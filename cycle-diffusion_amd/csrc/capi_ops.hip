// The cd_op_* half of the extern "C" boundary (include/cyclediff.h): one kernel, or one building block of the engine, per
// entry point, on operands the caller hands in. They exist for the parity tests (tests/_ops.py) and the micro-benchmarks;
// the Python API itself calls only cd_op_lowpass, cd_op_gauss, cd_op_cross_attention_maps, cd_op_automask_reduce,
// cd_op_local_blend_mask and cd_op_bench_mfma_sustained. No network forward and no sampler loop runs through this file.
//
// A new test entry stages its operands with the helpers below and writes nothing of the kind itself:
//   dense        op_rows16 (fp32 [rows][C] -> 16-bit), op_image16 (fp32 NCHW -> 16-bit NHWC Act)
//   NaN-guarded  op_nan_rows16 + op_put_cols16 (16-bit rows), op_nan_buffer + op_put_cols / op_upload_rows (fp32 rows),
//                op_upload_nhwc16 / op_upload_nhwc / op_upload_nhwc_split (images) - a read outside the operand shows
//   in place     op_rows_view (an Act over bytes that already lie as the kernel reads them)
//   results      op_download_nchw (queued), op_download (raw words, waits, range guard)
//   the rest     conv_out_hw, prec_ctx
#include "capi_internal.h"

namespace {

// ---- dense uploads
// fp32 [rows][C] -> a fresh 16-bit [rows][C], rounded by launch_nchw_to_nhwc
bf16_t* op_rows16(cd_engine* h, const float* src, int64_t rows, int C) {
  bf16_t* d = (bf16_t*)h->arena.alloc((size_t)rows * C * 2);
  launch_nchw_to_nhwc(h->st, src, d, (int)rows, C, 1, C, 1.f, 0.f, 0);
  return d;
}
// fp32 NCHW [B][C][H*W] -> a fresh 16-bit NHWC activation of Cpad channels
Act op_image16(Ctx& c, const float* x, int B, int C, int H, int W, int Cpad) {
  Act a = alloc_act(c, B, H, W, Cpad);
  launch_nchw_to_nhwc(c.st, x, a.p, B, C, H * W, Cpad, 1.f, 0.f, 0);
  return a;
}

// ---- NaN-guarded rows: the operand lies in columns of a wider buffer whose every other element is NaN
// 16-bit: the buffer starts as 0xFF bytes (a NaN in fp16 and in bf16) and carries one more 64-row block of them behind its
// last row, so a read outside the operand columns / rows shows in the result
bf16_t* op_nan_rows16(cd_engine* h, int64_t rows, int ld) {
  const size_t bytes = (size_t)(rows + 64) * ld * 2;
  bf16_t* t = (bf16_t*)h->arena.alloc(bytes);
  HIP_CHECK(hipMemsetAsync(t, 0xFF, bytes, h->st));
  return t;
}
float* op_nan_buffer(cd_engine* h, size_t n) {
  float* t = (float*)h->arena.alloc(n * sizeof(float));
  launch_fill_f32(h->st, t, __builtin_nanf(""), (int64_t)n);
  return t;
}
// columns [col0, col0 + C) of dst [rows][ld] (16-bit) <- fp32 src [rows][C], rounded by launch_nchw_to_nhwc
void op_put_cols16(cd_engine* h, bf16_t* dst, int ld, int col0, const float* src, int64_t rows, int C) {
  ArenaScope tmp_scope(h->arena);  // stream order: the copy below has read tmp before any later kernel reuses the space
  const bf16_t* tmp = op_rows16(h, src, rows, C);
  HIP_CHECK(hipMemcpy2DAsync(dst + col0, (size_t)ld * 2, tmp, (size_t)C * 2, (size_t)C * 2, (size_t)rows,
                             hipMemcpyDeviceToDevice, h->st));
}
// columns [col0, col0 + C) of dst [rows][ld] <- src [rows][C]
void op_put_cols(cd_engine* h, float* dst, int ld, int col0, const float* src, int64_t rows, int C) {
  HIP_CHECK(hipMemcpy2DAsync(dst + col0, (size_t)ld * 4, src, (size_t)C * 4, (size_t)C * 4, (size_t)rows,
                             hipMemcpyDeviceToDevice, h->st));
}

// ---- a rows-shaped activation [B][T][C] with row stride ld over bytes that already lie as the kernel reads them
Act op_rows_view(const void* p, int B, int T, int C, int ld, bool f32) {
  Act a; a.p = (bf16_t*)const_cast<void*>(p); a.B = B; a.H = T; a.W = 1; a.C = C; a.ld = ld; a.f32 = f32;
  return a;
}
// fp32 [rows][C] -> [rows][C + pad], NaN in the pad columns
Act op_upload_rows(cd_engine* h, const float* x, int64_t rows, int C, int pad) {
  const int ld = C + pad;
  float* t = op_nan_buffer(h, (size_t)rows * ld);
  op_put_cols(h, t, ld, 0, x, rows, C);
  return op_rows_view(t, (int)rows, 1, C, ld, true);
}

// ---- NaN-guarded images
// x fp32 NCHW [B][C][HW] as it is when ld == C, else a staging copy with ld channels per image: [C, Czero) hold 0, [Czero, ld) NaN
const float* op_nchw_guarded(cd_engine* h, const float* x, int B, int C, int Czero, int ld, int HW) {
  if (ld == C) return x;
  float* t = op_nan_buffer(h, (size_t)B * ld * HW);
  if (Czero > C)
    HIP_CHECK(hipMemset2DAsync(t + (size_t)C * HW, (size_t)ld * HW * 4, 0, (size_t)(Czero - C) * HW * 4, B, h->st));
  HIP_CHECK(hipMemcpy2DAsync(t, (size_t)ld * HW * 4, x, (size_t)C * HW * 4, (size_t)C * HW * 4, B, hipMemcpyDeviceToDevice,
                             h->st));
  return t;
}
// fp32 NCHW -> fp32 NHWC with row stride ld: channels [C, Czero) hold 0 (the weights' channel padding), [Czero, ld) NaN
Act op_upload_nhwc(cd_engine* h, const float* x, int B, int C, int Czero, int ld, int H, int W) {
  const int HW = H * W;
  Act a; a.B = B; a.H = H; a.W = W; a.C = Czero; a.ld = ld; a.f32 = true;
  a.p = (bf16_t*)h->arena.alloc((size_t)B * HW * ld * sizeof(float));
  launch_nchw_to_nhwc_f32(h->st, op_nchw_guarded(h, x, B, C, Czero, ld, HW), a.pf(), B, ld, HW, ld, 1.f, 0.f);
  return a;
}
// fp32 NCHW -> 16-bit NHWC with row stride ld: channels [C, ld) NaN; with Czero > C, [C, Czero) hold 0 and [Czero, ld) NaN
Act op_upload_nhwc16(cd_engine* h, const float* x, int B, int C, int ld, int H, int W, int Czero = 0) {
  const int HW = H * W;
  if (Czero < C) Czero = C;
  Act a; a.B = B; a.H = H; a.W = W; a.C = C; a.ld = ld;
  a.p = (bf16_t*)h->arena.alloc((size_t)B * HW * ld * sizeof(bf16_t));
  launch_nchw_to_nhwc(h->st, op_nchw_guarded(h, x, B, C, Czero, ld, HW), a.p, B, ld, HW, ld, 1.f, 0.f, 0);
  return a;
}
// the split form straight from NCHW (k_nchw_to_nhwc_split, as the U-Net input is uploaded): [pixel][hi(Cpad) | lo(Cpad)]
Act op_upload_nhwc_split(cd_engine* h, const float* x, int B, int C, int Cpad, int H, int W) {
  Act a; a.B = B; a.H = H; a.W = W; a.C = Cpad; a.ld = 2 * Cpad; a.f32 = true; a.split = true;
  a.p = (bf16_t*)h->arena.alloc((size_t)B * H * W * 2 * Cpad * sizeof(bf16_t));
  launch_nchw_to_nhwc_f32(h->st, x, a.pf(), B, C, H * W, Cpad, 1.f, 0.f, 1, h->overflow_dev);
  return a;
}

// ---- results
// rows [B * HW][ld] (16-bit, or fp32 when f32) -> the caller's fp32 NCHW [B][C][HW]; queued on the stream, not waited for
void op_download_nchw(cd_engine* h, const void* p, bool f32, int ld, float* y, int B, int C, int HW) {
  launch_nhwc_to_nchw(h->st, p, f32 ? 1 : 0, ld, y, B, C, HW, 1.f, 0.f);
}
// a result of `floats` 4-byte words (fp32 rows, or the fp16 pairs of the split mode: the same bytes) -> y; the range guard
void op_download(cd_engine* h, const Act& o, size_t floats, void* y) {
  HIP_CHECK(hipMemcpyAsync(y, o.p, floats * 4, hipMemcpyDeviceToDevice, h->st));
  HIP_CHECK(hipStreamSynchronize(h->st));
  h->check_overflow();
}

// ---- the rest
// output grid of a conv on an H x W input (nearest x2 upsampled first when `up`); asym = pad 0 / 1 (right and bottom only)
void conv_out_hw(int H, int W, int KH, int KW, int stride, int pad, bool asym, bool up, int* Ho, int* Wo) {
  const int Hin = up ? 2 * H : H, Win = up ? 2 * W : W;
  *Ho = asym ? (Hin + 1 - KH) / stride + 1 : (Hin + 2 * pad - KH) / stride + 1;
  *Wo = asym ? (Win + 1 - KW) / stride + 1 : (Win + 2 * pad - KW) / stride + 1;
}
// the Ctx a network of this precision runs under: 0 = 16-bit, 1 = fp32, 2 = fp32 split
Ctx prec_ctx(cd_engine* h, int precision) {
  Ctx c = h->ctx();
  c.f32 = precision != 0; c.x3 = precision == 2;
  return c;
}

void op_conv2d(cd_handle h, const float* x0, int C0, const float* x1, int C1, int B, int H, int W,
               const void* packed_w, int N, int KH, int KW, int stride, int pad, int asym_pad, int up,
               const float* bias, const float* rowvec, const float* resid, int act, int tile, bool out16,
               float* y, float* stats) {
  CD_CHECK(h && x0 && packed_w && y, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  if (up && out16) {  // an Upsample layer of the 16-bit path: give the packed weight its phase matrices, as the U-Net does at load
    ConvW* pw = (ConvW*)const_cast<void*>(packed_w);
    h->op_params.add_up_phase(pw);
    h->op_params.refresh_up_phase(h->st, pw);
  }
  ConvW w = *(const ConvW*)packed_w;
  CD_CHECK(w.N == N && w.KH == KH && w.KW == KW, "packed weight does not match the call");
  w.b = const_cast<float*>(bias);
  Act a0 = op_image16(c, x0, B, C0, H, W, x1 ? C0 : round_up(C0, 32));
  Act a1;
  if (x1) a1 = op_image16(c, x1, B, C1, H, W, C1);
  ConvOpts o; o.stride = stride; o.pad = pad; o.asym = asym_pad != 0; o.up = up != 0; o.tile = tile;
  if (act & 0x400) {  // LayerNorm (no gain / bias) of the input rows inside the kernel: streaming linear kernel only
    CD_CHECK(out16 && conv_ln_fold_available(c, w, (int64_t)B * H * W) , "LayerNorm fold needs tile 30 shapes");
    o.ln_fold = true;
    act &= ~0x400;
  }
  o.act = act;
  o.out_f32 = !out16;
  o.want_stats = stats != nullptr;
  int Ho, Wo;
  conv_out_hw(H, W, KH, KW, stride, pad, asym_pad != 0, up != 0, &Ho, &Wo);
  const int Nout = w.geglu ? N / 2 : N;
  if (rowvec) { o.rowvec = rowvec; o.rowvec_ld = N; o.rows_per_vec = Ho * Wo; }
  Act r;
  if (resid) {
    r = op_image16(c, resid, B, Nout, Ho, Wo, Nout);
    o.resid = &r;
  }
  Act out = conv_fwd(c, w, a0, x1 ? &a1 : nullptr, o);
  op_download_nchw(h, out.p, !out16, out.ld, y, B, Nout, Ho * Wo);
  if (stats) {
    CD_CHECK(out.stats, "this convolution produces no GroupNorm statistics (GEGLU, or rows %% 32 != 0)");
    HIP_CHECK(hipMemcpyAsync(stats, out.stats, (size_t)(out.rows() / 32) * 2 * Nout * sizeof(float),
                             hipMemcpyDeviceToDevice, h->st));
  }
}

void op_cross_attention_ctrl(cd_engine* h, const float* q_own, const float* q_src, const float* k_own,
                             const float* k_src, const float* v_own, const float* mapper, const float* alpha,
                             const float* weight, int B, int B_src, int B_ctrl, int H, int Tq, int L, int L_buf, int D,
                             float scale, int q_log2, int opad, float* o) {
  CD_CHECK(h && q_own && q_src && k_own && k_src && v_own && mapper && alpha && weight && o, "bad argument");
  CD_CHECK(B > 0 && B_src > 0 && B_ctrl > 0 && H > 0 && Tq > 0 && D > 0 && L > 0 && L_buf >= L, "bad argument");
  CD_CHECK(opad >= 0 && opad % 4 == 0, "opad: a multiple of 4 elements");
  ArenaScope arena_scope(h->arena);
  const int C = H * D, ldo = C + opad;
  CtrlAttnParams p;
  p.q_own = op_rows16(h, q_own, (int64_t)B * Tq, C); p.q_src = op_rows16(h, q_src, (int64_t)B_src * Tq, C);
  p.k_own = op_rows16(h, k_own, (int64_t)B * L_buf, C); p.k_src = op_rows16(h, k_src, (int64_t)B_src * L_buf, C);
  const bf16_t* vb16 = op_rows16(h, v_own, (int64_t)B * L, C);
  bf16_t* va = (bf16_t*)h->arena.alloc((size_t)B * L * C * 2);
  bf16_t* vb = (bf16_t*)h->arena.alloc((size_t)B * L * C * 2);
  launch_ctrl_values(h->st, vb16, mapper, alpha, weight, B, B_ctrl, L, C, va, vb);
  bf16_t* ob = op_nan_rows16(h, (int64_t)B * Tq, ldo);
  p.va = va; p.vb = vb; p.o = ob;
  p.B = B; p.B_src = B_src; p.H = H; p.Tq = Tq; p.L = L; p.D = D;
  p.ldq = C; p.ldk = C; p.ldv = C; p.ldo = ldo;
  p.q_bs = (int64_t)Tq * C; p.k_bs = (int64_t)L_buf * C; p.v_bs = (int64_t)L * C; p.o_bs = (int64_t)Tq * ldo;
  p.scale = scale; p.q_log2 = q_log2 != 0;
  launch_cross_attention_ctrl(h->st, p);
  op_download_nchw(h, ob, false, ldo, o, B * Tq, ldo, 1);
}

}  // namespace

extern "C" {

int cd_op_pack_conv_weight(cd_handle h, const float* w_host, int N, int Cin, int KH, int KW, int geglu,
                           void** packed_dev, int* Npad, int* Cpad) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && w_host && packed_dev, "bad argument");
  static int counter = 0;
  ConvW* c = h->op_params.new_conv(N, Cin, KH, KW, false, geglu != 0);
  const std::string name = "op." + std::to_string(counter++);
  h->op_params.conv_weight(name, c);
  int64_t shape[4] = {N, Cin, KH, KW};
  h->op_params.load(h->st, name, w_host, 4, shape);
  *packed_dev = c;
  if (Npad) *Npad = c->Npad;
  if (Cpad) *Cpad = c->Cpad;
  CD_API_END
}

int cd_op_free(cd_handle, void*) { return 0; }  // op weights live until the engine is destroyed

int cd_op_conv2d(cd_handle h, const float* x0, int C0, const float* x1, int C1, int B, int H, int W,
                 const void* packed_w, int N, int KH, int KW, int stride, int pad, int asym_pad, int up,
                 const float* bias, const float* rowvec, const float* resid, int act, int tile, float* y) {
  CD_API_BEGIN
  enter_engine(h);
  op_conv2d(h, x0, C0, x1, C1, B, H, W, packed_w, N, KH, KW, stride, pad, asym_pad, up, bias, rowvec, resid, act, tile,
            false, y, nullptr);
  CD_API_END
}

int cd_op_conv2d_16(cd_handle h, const float* x0, int C0, const float* x1, int C1, int B, int H, int W,
                    const void* packed_w, int N, int KH, int KW, int stride, int pad, int asym_pad, int up,
                    const float* bias, const float* rowvec, const float* resid, int act, int tile, float* y,
                    float* stats) {
  CD_API_BEGIN
  enter_engine(h);
  op_conv2d(h, x0, C0, x1, C1, B, H, W, packed_w, N, KH, KW, stride, pad, asym_pad, up, bias, rowvec, resid, act, tile,
            true, y, stats);
  CD_API_END
}

int cd_op_up_phase_reorder(cd_handle h, const float* x, int B, int C, int H, int W, float* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  Act a = op_image16(c, x, 4 * B, C, H, W, C);  // rows in (image, phase, y, x) order, as the phase-form GEMM leaves them
  Act o = alloc_act(c, B, 2 * H, 2 * W, C);
  launch_up_phase_reorder(h->st, a.p, o.p, B, H, W, C, o.ld);
  op_download_nchw(h, o.p, false, o.ld, y, B, C, 4 * H * W);
  CD_API_END
}

int cd_op_last_gemm_config(cd_handle h, int* tile_id, int* bk, int* splitk, int* chm, int* tile_group) {
  CD_API_BEGIN
  CD_CHECK(h, "bad argument");
  const GemmLaunchInfo li = conv_gemm_last_launch();
  if (tile_id) *tile_id = li.tile_id;
  if (bk) *bk = li.bk;
  if (splitk) *splitk = li.splitk;
  if (chm) *chm = li.chm;
  if (tile_group) *tile_group = li.tile_group;
  CD_API_END
}

int cd_op_groupnorm(cd_handle h, const float* x, int B, int C, int H, int W, int G, float eps,
                    const float* gamma, const float* beta, const float* film, int silu, float* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && G == 32, "bad argument (G must be 32)");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  Act a = op_image16(c, x, B, C, H, W, C);
  GNW w; w.g = const_cast<float*>(gamma); w.b = const_cast<float*>(beta); w.C = C; w.eps = eps;
  Act o = groupnorm_fwd(c, w, a, nullptr, silu != 0, film, film ? 2 * C : 0);
  op_download_nchw(h, o.p, false, o.ld, y, B, C, H * W);
  CD_API_END
}

// GroupNorm as the networks call it (groupnorm_fwd on the precision they run): one source or a channel concat of two, each
// with its own row stride C + pad (pad columns hold NaN: a read past C shows in the result), the producing convs' block
// statistics handed in by the caller (Act::stats), a FiLM row per image or one shared row (film_ld = 0)
int cd_op_groupnorm_ex(cd_handle h, const float* x0, int C0, int pad0, const float* x1, int C1, int pad1, int B, int H,
                       int W, float eps, const float* gamma, const float* beta, const float* film, int film_ld, int silu,
                       const float* stats0, const float* stats1, int precision, void* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x0 && gamma && beta && y && B > 0 && H > 0 && W > 0 && C0 > 0 && pad0 >= 0 && pad1 >= 0, "bad argument");
  CD_CHECK(x1 ? C1 > 0 : (C1 == 0 && !stats1), "bad argument (second source)");
  CD_CHECK(precision >= 0 && precision <= 2 && film_ld >= 0, "bad argument (precision 0 = 16-bit, 1 = fp32, 2 = fp32 split)");
  const int align = precision ? 4 : 8;  // the kernels' vector width in elements
  CD_CHECK((C0 + pad0) % align == 0 && (C1 + pad1) % align == 0, "row strides must be multiples of %d elements", align);
  ArenaScope arena_scope(h->arena);
  Ctx c = prec_ctx(h, precision);
  const int HW = H * W, C = C0 + C1;
  Act a0 = c.f32 ? op_upload_nhwc(h, x0, B, C0, C0, C0 + pad0, H, W) : op_upload_nhwc16(h, x0, B, C0, C0 + pad0, H, W);
  a0.stats = const_cast<float*>(stats0);
  Act a1;
  if (x1) {
    a1 = c.f32 ? op_upload_nhwc(h, x1, B, C1, C1, C1 + pad1, H, W) : op_upload_nhwc16(h, x1, B, C1, C1 + pad1, H, W);
    a1.stats = const_cast<float*>(stats1);
  }
  GNW w; w.g = const_cast<float*>(gamma); w.b = const_cast<float*>(beta); w.C = C; w.eps = eps;
  Act o = groupnorm_fwd(c, w, a0, x1 ? &a1 : nullptr, silu != 0, film, film_ld);
  if (precision == 2) {  // the raw [rows][hi(C) | lo(C)] fp16 pairs, and the range guard of the split representation
    CD_CHECK(o.split && o.ld == 2 * C, "groupnorm: split output expected");
    op_download(h, o, (size_t)B * HW * C, y);
  } else {
    op_download_nchw(h, o.p, c.f32, o.ld, (float*)y, B, C, HW);
  }
  CD_API_END
}

int cd_op_layernorm(cd_handle h, const float* x, int rows, int C, const float* gamma, const float* beta,
                    float eps, float* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y, "bad argument");
  ArenaScope arena_scope(h->arena);
  const bf16_t* a = op_rows16(h, x, rows, C);
  bf16_t* o = (bf16_t*)h->arena.alloc((size_t)rows * C * 2);
  launch_layernorm(h->st, a, C, o, C, rows, C, gamma, beta, eps);
  op_download_nchw(h, o, false, C, y, rows, C, 1);
  CD_API_END
}

int cd_op_st_entry(cd_handle h, const float* x, int B, int H, int W, const float* gn_gamma, const float* gn_beta,
                   float gn_eps, const void* w_in, const float* b_in, const float* ln_gamma, const float* ln_beta,
                   const void* w_qk, const void* w_v, const float* v_bias, int stages, float* h_out, float* qk_out,
                   float* vt_out, int* stages_run) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && gn_gamma && gn_beta && w_in && ln_gamma && ln_beta && w_qk && w_v && h_out && qk_out && vt_out &&
               B > 0 && H > 0 && W > 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  const int C = 320, T = H * W;
  ConvW win = *(const ConvW*)w_in;
  win.b = const_cast<float*>(b_in);
  StEntryW w;
  w.norm.g = const_cast<float*>(gn_gamma); w.norm.b = const_cast<float*>(gn_beta); w.norm.C = C; w.norm.eps = gn_eps;
  w.ln1.g = const_cast<float*>(ln_gamma); w.ln1.b = const_cast<float*>(ln_beta); w.ln1.C = C;
  w.proj_in = &win; w.qk1 = (const ConvW*)w_qk; w.v1 = (const ConvW*)w_v;
  CD_CHECK(win.N == C && win.Cpad == C && w.qk1->N == 2 * C && w.qk1->Cpad == C && w.v1->N == C && w.v1->Cpad == C,
           "transformer entry: 320-channel weights expected");
  w.vbias = v_bias;
  {  // storage of the derived weights: one pair per (w_qk, w_v) of this engine, refilled by every call (op weights live
     // until the engine is destroyed, and the norm / bias vectors behind the same handles may differ from call to call)
    const auto key = std::make_pair(w_qk, w_v);
    auto it = h->op_st_entry.find(key);
    if (it == h->op_st_entry.end()) {
      st_entry_alloc(h->op_params, w);
      it = h->op_st_entry.emplace(key, std::make_pair(w.qkv, w.qkv_ln)).first;
    }
    w.qkv = it->second.first; w.qkv_ln = it->second.second;
  }
  st_entry_refresh(h->st, w);
  Act a = op_image16(c, x, B, C, H, W, C);
  if (stages < 0) stages = st_entry_stages();
  const StEntryOut r = st_entry_fwd(c, w, a, stages);
  if (stages_run) *stages_run = r.stages;
  op_download_nchw(h, r.h.p, false, r.h.ld, h_out, B, C, T);
  op_download_nchw(h, r.qk.p, false, r.qk.ld, qk_out, B, 2 * C, T);
  op_download_nchw(h, r.vt, false, r.Tpad, vt_out, B * C, r.Tpad, 1);  // [B][C][Tpad] as it is
  CD_API_END
}

int cd_op_attention(cd_handle h, const float* q, const float* k, const float* v, int B, int H, int Tq,
                    int Tk, int D, float scale, int use_transpose_kernel, float* o) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && q && k && v && o, "bad argument");
  ArenaScope arena_scope(h->arena);
  const int C = H * D, Tpad = round_up(Tk, 64);
  const bf16_t* qb = op_rows16(h, q, (int64_t)B * Tq, C);
  const bf16_t* kb = op_rows16(h, k, (int64_t)B * Tk, C);
  const bf16_t* vb = op_rows16(h, v, (int64_t)B * Tk, C);
  bf16_t* ob = (bf16_t*)h->arena.alloc((size_t)B * Tq * C * 2);
  AttnParams p;
  p.q = qb; p.k = kb; p.o = ob; p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk; p.D = D;
  p.ldq = C; p.ldk = C; p.ldo = C; p.q_bs = (int64_t)Tq * C; p.k_bs = (int64_t)Tk * C; p.o_bs = (int64_t)Tq * C;
  p.scale = scale;
  if (use_transpose_kernel) {  // V^T [B][H][D][Tpad] layout (k_transpose_v), else token-major V (LDS transpose reads)
    bf16_t* vt = (bf16_t*)h->arena.alloc((size_t)B * C * Tpad * 2);
    launch_transpose_v(h->st, vb, C, (int64_t)Tk * C, vt, B, H, Tk, D, D, Tpad);
    p.vt = vt; p.vt_dpad = D; p.vt_tpad = Tpad;
  } else {
    p.v = vb; p.ldv = C; p.v_bs = (int64_t)Tk * C;
  }
  launch_attention(h->st, p);
  op_download_nchw(h, ob, false, C, o, B * Tq, C, 1);
  CD_API_END
}

int cd_op_attention_ex(cd_handle h, const float* q, const float* k, const float* v, int B, int H, int Tq, int Tk, int D,
                       int layout, int pad, int v_transposed, int d_extra, int t_extra, float scale, int q_log2,
                       const float* obias, int causal, int opad, float* o) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && q && k && v && o && B > 0 && H > 0 && Tq > 0 && Tk > 0 && D > 0 && D % 8 == 0, "bad argument");
  CD_CHECK(layout >= 0 && layout <= 2, "bad argument (layout 0 = q, k, v apart, 1 = q | k in one tensor, 2 = q | k | v)");
  CD_CHECK(layout == 0 || Tq == Tk, "a fused q | k (| v) tensor needs Tq = Tk");
  CD_CHECK(!(layout == 2 && v_transposed), "the fused q | k | v tensor carries V token-major");
  CD_CHECK(pad >= 0 && pad % 8 == 0, "pad: a multiple of 8 elements");
  CD_CHECK(opad >= 0 && opad % 4 == 0, "opad: a multiple of 4 elements");
  CD_CHECK(d_extra >= 0 && t_extra >= 0 && (v_transposed || (d_extra == 0 && t_extra == 0)),
           "d_extra / t_extra pad V^T only");
  ArenaScope arena_scope(h->arena);
  const int C = H * D;
  const int64_t rq = (int64_t)B * Tq, rk = (int64_t)B * Tk;
  AttnParams p;
  const bf16_t* vb;
  int ldv;
  if (layout == 0) {  // every tensor padded, and no two row strides equal: a stride taken from the wrong operand shows
    const int lq = C + pad, lk = C + 2 * pad, lv = C + 3 * pad;
    bf16_t* qb = op_nan_rows16(h, rq, lq);
    bf16_t* kb = op_nan_rows16(h, rk, lk);
    bf16_t* vv = op_nan_rows16(h, rk, lv);
    op_put_cols16(h, qb, lq, 0, q, rq, C);
    op_put_cols16(h, kb, lk, 0, k, rk, C);
    op_put_cols16(h, vv, lv, 0, v, rk, C);
    p.q = qb; p.k = kb; p.ldq = lq; p.ldk = lk; vb = vv; ldv = lv;
  } else {
    const int n = layout + 1, ld = n * C + pad;  // q | k (| v) as column blocks of one tensor
    bf16_t* t = op_nan_rows16(h, rq, ld);
    op_put_cols16(h, t, ld, 0, q, rq, C);
    op_put_cols16(h, t, ld, C, k, rq, C);
    p.q = t; p.k = t + C; p.ldq = p.ldk = ld;
    if (layout == 2) {
      op_put_cols16(h, t, ld, 2 * C, v, rq, C);
      vb = t + 2 * C; ldv = ld;
    } else {
      bf16_t* vv = op_nan_rows16(h, rk, C + pad);
      op_put_cols16(h, vv, C + pad, 0, v, rk, C);
      vb = vv; ldv = C + pad;
    }
  }
  const int ldo = C + opad;
  bf16_t* ob = op_nan_rows16(h, rq, ldo);
  p.o = ob; p.ldo = ldo;
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk; p.D = D;
  p.q_bs = (int64_t)Tq * p.ldq; p.k_bs = (int64_t)Tk * p.ldk; p.o_bs = (int64_t)Tq * ldo;
  p.scale = scale; p.q_log2 = q_log2 != 0; p.obias = obias; p.causal = causal != 0;
  if (v_transposed) {  // V^T [B][H][D + d_extra][round_up(Tk, 64) + 64 t_extra]: its padding is launch_transpose_v's zeros
    const int Dpad = D + d_extra, Tpad = round_up(Tk, 64) + 64 * t_extra;
    bf16_t* vt = (bf16_t*)h->arena.alloc((size_t)B * H * Dpad * Tpad * 2);
    launch_transpose_v(h->st, vb, ldv, (int64_t)Tk * ldv, vt, B, H, Tk, D, Dpad, Tpad);
    p.vt = vt; p.vt_dpad = Dpad; p.vt_tpad = Tpad;
  } else {
    p.v = vb; p.ldv = ldv; p.v_bs = (int64_t)Tk * ldv;
  }
  launch_attention(h->st, p);
  op_download_nchw(h, ob, false, ldo, o, (int)rq, ldo, 1);
  CD_API_END
}

int cd_op_cross_attention_ctrl(cd_handle h, const float* q_own, const float* q_src, const float* k_own, const float* k_src,
                               const float* v_own, const float* mapper, const float* alpha, const float* weight, int B,
                               int B_src, int B_ctrl, int H, int Tq, int L, int L_buf, int D, float scale, float* o) {
  CD_API_BEGIN
  enter_engine(h);
  op_cross_attention_ctrl(h, q_own, q_src, k_own, k_src, v_own, mapper, alpha, weight, B, B_src, B_ctrl, H, Tq, L, L_buf, D,
                          scale, 0, 0, o);
  CD_API_END
}

int cd_op_cross_attention_ctrl_ex(cd_handle h, const float* q_own, const float* q_src, const float* k_own, const float* k_src,
                                  const float* v_own, const float* mapper, const float* alpha, const float* weight, int B,
                                  int B_src, int B_ctrl, int H, int Tq, int L, int L_buf, int D, float scale, int q_log2,
                                  int opad, float* o) {
  CD_API_BEGIN
  enter_engine(h);
  op_cross_attention_ctrl(h, q_own, q_src, k_own, k_src, v_own, mapper, alpha, weight, B, B_src, B_ctrl, H, Tq, L, L_buf, D,
                          scale, q_log2, opad, o);
  CD_API_END
}

// k_cross_attention_maps on caller-built operands: q [B, Tq, H*D], k [B, L_buf, H*D] (rows L .. L_buf-1 must not be read),
// sel [B_sel, N, L] -> maps [B, N, Tq]
int cd_op_cross_attention_maps(cd_handle h, const float* q, const float* k, const float* sel, int B, int B_sel, int H,
                               int Tq, int L, int L_buf, int D, int N, float scale, int q_log2, float* maps) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && q && k && sel && maps, "bad argument");
  CD_CHECK(B > 0 && B_sel > 0 && H > 0 && Tq > 0 && D > 0 && L > 0 && L_buf >= L, "bad argument");
  ArenaScope arena_scope(h->arena);
  const int C = H * D;
  WordMapParams p;
  p.q = op_rows16(h, q, (int64_t)B * Tq, C); p.k = op_rows16(h, k, (int64_t)B * L_buf, C); p.sel = sel; p.maps = maps;
  p.B = B; p.B_sel = B_sel; p.H = H; p.Tq = Tq; p.L = L; p.D = D; p.N = N;
  p.ldq = C; p.ldk = C; p.q_bs = (int64_t)Tq * C; p.k_bs = (int64_t)L_buf * C;
  p.scale = scale; p.q_log2 = q_log2 != 0;
  launch_cross_attention_maps(h->st, p);
  CD_API_END
}

// y = phi_N(x) through the two ILVR kernels (x' = 0, qa = 1, qb = 0)
int cd_op_lowpass(cd_handle h, const float* x, int B, int C, int R, int down_n, float* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && B > 0 && C > 0 && R > 0, "bad argument");
  check_lowpass_geometry(R, down_n);
  ArenaScope arena_scope(h->arena);
  const int r = R / down_n;
  IlvrArgs iv;
  iv.out = y; iv.y = x; iv.y_bmod = B;
  iv.B = B; iv.C = C; iv.R = R;
  iv.D = upload_taps(h, R, r);
  iv.U = upload_taps(h, r, R);
  iv.T = (float*)h->arena.alloc((size_t)B * C * r * r * sizeof(float));
  iv.vec4 = (R % 4 == 0 && aligned16(x) && aligned16(y)) ? 1 : 0;
  launch_ilvr_down(h->st, iv);
  launch_ilvr_up_add(h->st, iv);
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

int cd_op_softmax_rows(cd_handle h, const float* s, int64_t rows, int cols, float* p) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && s && p, "bad argument");
  ArenaScope arena_scope(h->arena);
  bf16_t* pb = (bf16_t*)h->arena.alloc((size_t)rows * cols * 2);
  launch_softmax_rows(h->st, s, cols, pb, cols, rows, cols);
  op_download_nchw(h, pb, false, cols, p, (int)rows, cols, 1);
  CD_API_END
}

int cd_op_timestep_embedding(cd_handle h, const float* t, int B, int dim, int mode, float* out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && t && out, "bad argument");
  launch_timestep_embedding(h->st, nullptr, 0, t, out, B, dim, mode);
  CD_API_END
}

int cd_op_sched_step(cd_handle h, int mode, int sched_kind, const cd_step_coef* coef_host, const float* x0,
                     float* xt, const float* eps_hat, int cfg, float guidance, const float* noise,
                     const float* eps_in, int is_last, int B, int C, int HW, float* z_slot) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && coef_host && xt, "bad argument");
  ArenaScope arena_scope(h->arena);
  const int64_t chw = (int64_t)C * HW;
  StepArgs a;
  a.x0 = x0; a.xt = xt;
  a.eh.p = eps_hat; a.eh.sb = chw; a.eh.sc = HW; a.eh.sp = 1; a.eh.cfg = cfg; a.eh.g = guidance;  // NCHW view
  a.geom.B = B; a.geom.C = C; a.geom.HW = HW; a.geom.tab = upload_coef(h, coef_host, 1);
  a.gauss.noise = noise;
  a.eps.p = eps_in; a.eps.bstride = chw;
  a.z.p = z_slot; a.z.bstride = chw;
  a.is_last = is_last;
  if (mode == 0) launch_init_xt(h->st, a);
  else if (mode == 1) launch_encode_step(h->st, sched_kind, a);
  else launch_decode_step(h->st, sched_kind, a);
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

// n draws of the counter-based generator, elements first .. first + n - 1 of (seed, stream), as the kernels take them
int cd_op_gauss(cd_handle h, uint64_t seed, uint32_t stream, int64_t first, int64_t n, float* out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && out && first >= 0 && n >= 0 && first <= INT64_MAX - n, "bad argument");
  GaussSrc g;
  g.seed = seed; g.stream = stream;
  if (n > 0) launch_gauss_fill(h->st, g, first, out, n);
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

// the reduction of cd_automask on caller-built predictions, fp32 [n, B, C, H, W] each
int cd_op_automask_reduce(cd_handle h, const float* eps_src, const float* eps_tgt, int n, int B, int C, int H, int W,
                          float ratio, float thr, int dilate, float* map_out, float* mean_out, float* keep_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && eps_src && eps_tgt && keep_out && B > 0 && C > 0 && H > 0 && W > 0, "bad argument");
  check_automask_params(n, ratio, thr, dilate);
  ArenaScope arena_scope(h->arena);
  const int HW = H * W;
  AutoMaskArgs m;
  m.B = B; m.C = C; m.H = H; m.W = W;
  m.e_src = eps_src; m.e_tgt = eps_tgt;
  m.sb = (int64_t)C * HW; m.sc = HW; m.sp = 1;  // NCHW view
  m.n_chunk = m.n_total = n; m.first = 1;
  m.ratio = ratio; m.thr = thr; m.dilate = dilate;
  m.nblk = automask_sum_blocks(HW);
  m.acc = (float*)h->arena.alloc((size_t)B * HW * 4);
  m.partial = (float*)h->arena.alloc((size_t)B * m.nblk * 4);
  m.map_out = map_out; m.mean_out = mean_out; m.keep_out = keep_out;
  launch_automask_accum(h->st, m);
  launch_automask_finish(h->st, m);
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

// one launch of k_local_blend_mask on caller-built sums
int cd_op_local_blend_mask(cd_handle h, const float* acc_src, const float* acc_tgt, int B, int Bd, int side, int f, int pool,
                           float thr, float* keep_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && acc_src && acc_tgt && keep_out && B > 0 && Bd > 0, "bad argument");
  CD_CHECK(Bd % B == 0, "local blend shape mismatch: %d decoder rows for %d source rows", Bd, B);
  LocalBlendMask lm;
  lm.acc_src = acc_src; lm.acc_tgt = acc_tgt; lm.keep = keep_out;
  lm.B = B; lm.Bd = Bd; lm.side = side; lm.f = f; lm.pool = pool; lm.thr = thr;
  launch_local_blend_mask(h->st, lm);
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

// one launch of k_window_gather on a caller's canvas; the 16-bit rows come back as fp32
int cd_op_window_gather(cd_handle h, const float* x, const int32_t* win_host, int n_win, int Bp, int C, int Hc, int Wc, int S,
                        int cpad, int dup, float* y_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y_out && Bp > 0 && C > 0 && cpad >= C && cpad % 8 == 0 && (dup == 0 || dup == 1), "bad argument");
  check_window_grid(win_host, n_win, Hc, Wc, S);
  ArenaScope arena_scope(h->arena);
  const int64_t n = (int64_t)(1 + dup) * n_win * Bp * S * S * cpad;
  CD_CHECK(n < (1ll << 31), "window gather op: %lld values", (long long)n);
  WindowGather g;
  g.x = x; g.y = (bf16_t*)h->arena.alloc((size_t)n * 2);
  g.win = (const int*)upload_table(h, win_host, (size_t)n_win * 2 * sizeof(int32_t));
  g.Bp = Bp; g.C = C; g.Hc = Hc; g.Wc = Wc; g.S = S; g.n_win = n_win; g.cpad = cpad; g.dup = dup;
  launch_window_gather(h->st, g);
  launch_nhwc_to_nchw(h->st, g.y, 0, 1, y_out, 1, 1, (int)n, 1.f, 0.f);  // the values as they lie, widened
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

// one launch of k_window_fuse (the C = ld = 4 form where it applies) on a caller's network output rows
int cd_op_window_fuse(cd_handle h, const float* e, const int32_t* win_host, int n_win, int Bp, int C, int Hc, int Wc, int S,
                      int ld, int parts, float* out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && e && out && Bp > 0 && C > 0 && ld >= C && parts >= 1, "bad argument");
  check_window_grid(win_host, n_win, Hc, Wc, S);
  ArenaScope arena_scope(h->arena);
  WindowFuse f;
  f.e = e; f.out = out;
  f.win = (const int*)upload_table(h, win_host, (size_t)n_win * 2 * sizeof(int32_t));
  f.Bp = Bp; f.C = C; f.Hc = Hc; f.Wc = Wc; f.S = S; f.n_win = n_win; f.ld = ld; f.parts = parts;
  launch_window_fuse(h->st, f);
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

// the masked step kernels on explicit tensors: mode 0 = k_mask_blend_init, 2 = k_decode_step_ddim<true> (blend = 0: last step)
int cd_op_sched_step_masked(cd_handle h, int mode, const cd_step_coef* coef_host, float* x, const float* eps_hat, int cfg,
                            float guidance, const float* eps_in, const float* mask, const float* src, int B_mask,
                            int mask_source, float qa, float qb, const float* mask_noise, int blend, int B, int C, int HW,
                            void* xin16_out, int cfg_dup) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && mask && src && B > 0 && C > 0 && HW > 0, "bad argument");
  CD_CHECK(B_mask > 0 && B % B_mask == 0, "mask shape mismatch: %d mask rows for a batch of %d", B_mask, B);
  CD_CHECK(mode == 0 || (coef_host && eps_hat), "bad argument");
  ArenaScope arena_scope(h->arena);
  const int64_t chw = (int64_t)C * HW;
  MaskBlend mk;
  mk.mask = mask; mk.src = src; mk.mask_bmod = mk.src_bmod = B_mask; mk.gauss.noise = mask_noise;
  if (mask_source == CD_MASK_QSAMPLE) {
    CD_CHECK(mask_noise, "q_sample mode needs the noise tensor here");
    const float q[2] = {qa, qb};
    mk.qtab = (const float2*)upload_table(h, q, sizeof(q));
  }
  StepArgs a;
  a.xt = x;
  a.geom.B = B; a.geom.C = C; a.geom.HW = HW;
  a.xin.xin = (bf16_t*)xin16_out; a.xin.cpad = C; a.xin.dup = cfg_dup;
  if (mode == 0) {
    launch_mask_blend_init(h->st, a, mk);
  } else {
    a.geom.tab = upload_coef(h, coef_host, 1);
    a.eh.p = eps_hat; a.eh.sb = chw; a.eh.sc = HW; a.eh.sp = 1; a.eh.cfg = cfg; a.eh.g = guidance;  // NCHW view
    a.eps.p = eps_in; a.eps.bstride = chw;
    launch_decode_step(h->st, CD_SCHED_DDIM, a, &mk, blend != 0);
  }
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

int cd_op_sega_guidance(cd_handle h, const float* eps_all, int Bd, int C, int HW, int E, int ld, float guidance,
                        const float* guidance_per_sample, const cd_sega_concept* concepts_host, int iteration,
                        float momentum_scale, float momentum_beta, float* nu, float* eps_out, float* tau_out,
                        int32_t* kept_out, float* mask_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && eps_all && nu && eps_out && tau_out && kept_out && Bd > 0 && C > 0 && HW > 0 && iteration >= 0, "bad argument");
  CD_CHECK(ld >= C, "semantic guidance: ld = %d below C = %d", ld, C);
  check_sega_params(concepts_host, E, (int64_t)C * HW, -1, momentum_scale, momentum_beta);
  ArenaScope arena_scope(h->arena);
  const int rows = (2 + E) * Bd;
  float* nhwc = (float*)h->arena.alloc((size_t)rows * HW * ld * 4);
  launch_nchw_to_nhwc_f32(h->st, eps_all, nhwc, rows, C, HW, ld, 1.f, 0.f);
  SegaStep a;
  a.eh.p = nhwc; a.eh.sb = (int64_t)HW * ld; a.eh.sc = 1; a.eh.sp = ld; a.eh.g = guidance; a.eh.gvec = guidance_per_sample;
  a.Bd = Bd; a.C = C; a.HW = HW; a.E = E;
  a.active = sega_active_mask(concepts_host, E, iteration);
  a.tab = (const SegaConcept*)upload_table(h, concepts_host, (size_t)E * sizeof(SegaConcept));
  a.abuf = (float*)h->arena.alloc((size_t)Bd * E * C * HW * 4);
  a.tau = tau_out; a.kept = kept_out; a.nu = nu; a.eps = eps_out; a.mask_out = mask_out;
  a.s_m = momentum_scale; a.beta = momentum_beta;
  HIP_CHECK(hipMemsetAsync(tau_out, 0, (size_t)Bd * E * 4, h->st));
  HIP_CHECK(hipMemsetAsync(kept_out, 0, (size_t)Bd * E * 4, h->st));
  launch_sega_guidance(h->st, a);
  HIP_CHECK(hipStreamSynchronize(h->st));
  CD_API_END
}

}  // extern "C"

// ------------------------------------------------------------------ hardware layout probes
namespace {
__global__ void k_probe_mfma(float* out) {
  // which=0: D = A.B with A[i][0] = i+1 (else 0), B[0][j] = 1  -> D[i][j] = i+1 (row map)
  //          then A[i][0] = 1, B[0][j] = j+1                   -> D[i][j] = j+1 (col map)
  const int lane = threadIdx.x & 63;
  bf16x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (lane < 32) { a[0] = (short)f2bf((float)(lane + 1)); b[0] = (short)f2bf(1.0f); }
  acc = CD_MFMA_32x32x16(a, b, acc);
  for (int r = 0; r < 16; ++r) out[lane * 16 + r] = acc[r];
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (lane < 32) { a[0] = (short)f2bf(1.0f); b[0] = (short)f2bf((float)(lane + 1)); }
  acc = CD_MFMA_32x32x16(a, b, acc);
  for (int r = 0; r < 16; ++r) out[1024 + lane * 16 + r] = acc[r];
  // k-slot check: A[i][k] = 1 for all i, only k = kk set; B[kk][j] = kk+1 -> D = sum over matching k
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int j = 0; j < 8; ++j) { a[j] = (short)f2bf(1.0f); b[j] = (short)f2bf((float)(8 * (lane >> 5) + j + 1)); }
  acc = CD_MFMA_32x32x16(a, b, acc);
  for (int r = 0; r < 16; ++r) out[2048 + lane * 16 + r] = acc[r];  // expect 1+2+...+16 = 136
}
__global__ void k_probe_tr(float* out) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[256];
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < 256; i += 64) lds[i] = f2bf((float)i);
  __syncthreads();
  uint2 v;
  const unsigned addr = (unsigned)(size_t)(lds) + lane * 8;
  asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
  out[lane * 4 + 0] = bf2f((bf16_t)(v.x & 0xffff));
  out[lane * 4 + 1] = bf2f((bf16_t)(v.x >> 16));
  out[lane * 4 + 2] = bf2f((bf16_t)(v.y & 0xffff));
  out[lane * 4 + 3] = bf2f((bf16_t)(v.y >> 16));
}
// The address pattern k_attention uses for its PV A operand (token-major V tile [64 keys][96] in LDS): 16 lanes fetch a
// 4-key x 16-d block, lane l must receive column d = dt*32 + (l & 31) of keys base + 4*(l >> 5) + 0..3.
__global__ void k_probe_tr_attn(float* out) {
  constexpr int VS = 96;
  __shared__ __attribute__((aligned(16))) bf16_t lds[64 * VS];
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < 64 * VS; i += 64) lds[i] = (bf16_t)((i / VS) * 64 + (i % VS < 64 ? i % VS : 0));  // raw key*64+d
  __syncthreads();
  typedef __attribute__((address_space(3))) bf16x4* lds4_t;
  const int half = lane >> 5;
  const int vtr_off = (4 * half + ((lane & 15) >> 2)) * VS + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  int n = 0;
  for (int sel = 0; sel < 2; ++sel) {  // (kh, s2, dt) = (0, 0, 0) and (1, 1, 1)
    const bf16_t* vr = lds + vtr_off + (sel * 32 + 16 * sel) * VS + sel * 32;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)vr);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(vr + 8 * VS));
    for (int j = 0; j < 4; ++j) out[lane * 16 + n++] = (float)(unsigned short)lo[j];
    for (int j = 0; j < 4; ++j) out[lane * 16 + n++] = (float)(unsigned short)hi[j];
  }
}

__global__ void k_fill_hash16(bf16_t* p, int64_t n, uint32_t seed, float scale) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t x = (uint32_t)i * 2654435761u + seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    p[i] = f2bf(((float)(x & 0xffff) / 32768.0f - 1.0f) * scale);  // uniform [-scale, scale): full-range data
  }
}
}  // namespace

extern "C" {

// Micro-benchmark of one conv / GEMM shape on synthetic full-range data: `iters` back-to-back launches
// between two HIP events on the engine stream. ms_out = average per launch.
int cd_op_bench_conv(cd_handle h, int B, int H, int W, int C0, int C1, int N, int k, int stride,
                     int up, int act, int tile, int iters, float* ms_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && ms_out && iters > 0, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  ConvW w;
  w.N = N; w.Cin = C0 + C1; w.KH = k; w.KW = k; w.Cpad = round_up(C0 + C1, 32); w.Npad = round_up(N, 128);
  w.geglu = (act == ACT_GEGLU);
  const size_t wn = (size_t)w.Npad * w.Ktot();
  w.w = (bf16_t*)h->arena.alloc(wn * 2);
  w.b = (float*)h->arena.alloc((size_t)w.Npad * 4);
  HIP_CHECK(hipMemsetAsync(w.b, 0, (size_t)w.Npad * 4, h->st));
  hipLaunchKernelGGL(k_fill_hash16, dim3(1024), dim3(256), 0, h->st, w.w, (int64_t)wn, 17u,
                     1.0f / sqrtf((float)w.Ktot()));
  if (k == 1 && w.Cpad == 320) {
    w.wfrag = (bf16_t*)h->arena.alloc(wn * 2);
    launch_pack_wfrag(h->st, w.w, w.Ktot(), w.wfrag, w.Npad);
  }
  const bool inplace_resid = (act & 0x100) != 0, want_stats = (act & 0x200) != 0;
  act &= 0xff;
  w.geglu = (act == ACT_GEGLU);
  Act a0 = alloc_act(c, B, H, W, C1 ? C0 : round_up(C0, 32));
  hipLaunchKernelGGL(k_fill_hash16, dim3(1024), dim3(256), 0, h->st, a0.p, (int64_t)a0.rows() * a0.C, 3u, 1.0f);
  Act a1;
  if (C1) {
    a1 = alloc_act(c, B, H, W, C1);
    hipLaunchKernelGGL(k_fill_hash16, dim3(1024), dim3(256), 0, h->st, a1.p, (int64_t)a1.rows() * a1.C, 5u, 1.0f);
  }
  ConvOpts o; o.stride = stride; o.pad = k / 2; o.up = up != 0; o.act = (act == ACT_GEGLU) ? ACT_NONE : act; o.tile = tile;
  Act ro;
  if (inplace_resid || want_stats) {  // the in-place residual update of the to_out / proj_out projections
    const int ho = up ? 2 * H : (H + 2 * o.pad - k) / stride + 1;
    ro = alloc_act(c, B, ho, ho, N, /*with_stats=*/true);
    hipLaunchKernelGGL(k_fill_hash16, dim3(1024), dim3(256), 0, h->st, ro.p, (int64_t)ro.rows() * ro.C, 7u, 0.01f);
    o.out = ro.p; o.out_ld = ro.ld;
    if (inplace_resid) o.resid = &ro;
    if (want_stats) o.out_stats = ro.stats_buf;
  }
  const size_t mk2 = h->arena.mark();
  conv_fwd(c, w, a0, C1 ? &a1 : nullptr, o);  // warm-up
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, h->st));
  for (int i = 0; i < iters; ++i) { h->arena.release(mk2); conv_fwd(c, w, a0, C1 ? &a1 : nullptr, o); }
  HIP_CHECK(hipEventRecord(e1, h->st));
  HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  *ms_out = ms / iters;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  CD_API_END
}

int cd_op_bench_mfma_sustained(cd_handle h, int target_ms, float* tflops_out, float* ghz_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && tflops_out && ghz_out && target_ms > 0 && target_ms <= 5000, "bad argument");
  launch_mfma_sustained(h->st, target_ms, tflops_out, ghz_out);
  CD_API_END
}

int cd_op_probe(cd_handle h, int which, const void* in, void* out, size_t n) {
  CD_API_BEGIN
  enter_engine(h);
  (void)in;
  CD_CHECK(h && out, "bad argument");
  if (which == 0) {
    CD_CHECK(n >= 3072 * sizeof(float), "probe 0 needs 3072 floats");
    hipLaunchKernelGGL(k_probe_mfma, dim3(1), dim3(64), 0, h->st, (float*)out);
  } else if (which == 1) {
    CD_CHECK(n >= 256 * sizeof(float), "probe 1 needs 256 floats");
    hipLaunchKernelGGL(k_probe_tr, dim3(1), dim3(64), 0, h->st, (float*)out);
  } else if (which == 2) {
    CD_CHECK(n >= 1024 * sizeof(float), "probe 2 needs 1024 floats");
    hipLaunchKernelGGL(k_probe_tr_attn, dim3(1), dim3(64), 0, h->st, (float*)out);
  } else {
    CD_CHECK(false, "unknown probe %d", which);
  }
  CD_API_END
}

// ------------------------------------------------------------------ single-kernel entry points of the fp32 path
// The engine's building blocks as the networks call them under a Ctx with f32 (precision 1) or f32 + x3 (precision 2, the
// split-fp16 mode) set. Operands are stored with row stride C + pad; the pad columns hold NaN, so a read past C shows.

int cd_op_pack_conv_weight_prec(cd_handle h, const float* w_host, int N, int Cin, int KH, int KW, int geglu,
                                void** packed_dev) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && w_host && packed_dev, "bad argument");
  static int counter = 0;
  ConvW* c = h->op_params_f32.new_conv(N, Cin, KH, KW, false, geglu != 0);
  const std::string name = "op32." + std::to_string(counter++);
  h->op_params_f32.conv_weight(name, c);
  int64_t shape[4] = {N, Cin, KH, KW};
  h->op_params_f32.load(h->st, name, w_host, 4, shape);  // synchronises: a weight outside the split range raises here
  h->check_overflow();
  *packed_dev = c;
  CD_API_END
}

int cd_op_conv2d_prec(cd_handle h, const float* x0, int C0, int pad0, const float* x1, int C1, int pad1, int B, int H, int W,
                      const void* packed_w, int N, int KH, int KW, int stride, int pad, int asym_pad, int up,
                      const float* bias, const float* rowvec, int rowvec_shared, const float* resid, int resid_pad, int act,
                      int raw_geglu, int tile, int precision, int via_split_rows, float alpha, float* y, float* stats) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x0 && packed_w && y && B > 0 && H > 0 && W > 0 && C0 > 0 && pad0 >= 0 && pad1 >= 0 && resid_pad >= 0,
           "bad argument");
  CD_CHECK(precision == 1 || precision == 2, "bad argument (precision 1 = fp32, 2 = fp32 split)");
  CD_CHECK(x1 ? C1 > 0 : C1 == 0, "bad argument (second source)");
  CD_CHECK(pad0 % 4 == 0 && pad1 % 4 == 0, "row padding must be a multiple of 4 elements");
  ArenaScope arena_scope(h->arena);
  Ctx c = prec_ctx(h, precision);
  ConvW w = *(const ConvW*)packed_w;
  CD_CHECK(w.f32 && w.N == N && w.KH == KH && w.KW == KW, "packed weight does not match the call");
  w.b = const_cast<float*>(bias);
  const int c0p = x1 ? C0 : round_up(C0, 32);
  Act a0, a1;
  const Act* second = nullptr;
  if (precision == 2 && !x1 && !via_split_rows) {
    CD_CHECK(pad0 == 0, "the split form has no row padding");
    a0 = op_upload_nhwc_split(h, x0, B, C0, c0p, H, W);
  } else {
    a0 = op_upload_nhwc(h, x0, B, C0, c0p, c0p + pad0, H, W);
    if (x1) a1 = op_upload_nhwc(h, x1, B, C1, C1, C1 + pad1, H, W);
    if (precision == 2) a0 = split_rows_f32_fwd(c, a0, x1 ? &a1 : nullptr);  // as unet_openai.hip feeds its skip projections
    else second = x1 ? &a1 : nullptr;
  }
  ConvOpts o; o.stride = stride; o.pad = pad; o.asym = asym_pad != 0; o.up = up != 0; o.tile = tile;
  o.act = act; o.alpha = alpha; o.raw_geglu = raw_geglu != 0; o.want_stats = stats != nullptr;
  int Ho, Wo;
  conv_out_hw(H, W, KH, KW, stride, pad, asym_pad != 0, up != 0, &Ho, &Wo);
  if (rowvec) { o.rowvec = rowvec; o.rowvec_ld = N; o.rows_per_vec = rowvec_shared ? B * Ho * Wo : Ho * Wo; }
  Act r;
  if (resid) {
    r = op_upload_nhwc(h, resid, B, N, N, N + resid_pad, Ho, Wo);
    o.resid = &r;
  }
  Act out = conv_fwd(c, w, a0, second, o);
  CD_CHECK(out.f32 && !out.split && out.C == N, "conv: fp32 output expected");
  op_download_nchw(h, out.p, true, out.ld, y, B, N, Ho * Wo);
  if (stats) {
    CD_CHECK(out.stats, "this convolution produces no GroupNorm statistics (fp32 without the split mode, or rows %% 32 != 0)");
    HIP_CHECK(hipMemcpyAsync(stats, out.stats, (size_t)(out.rows() / 32) * 2 * N * sizeof(float), hipMemcpyDeviceToDevice,
                             h->st));
  }
  HIP_CHECK(hipStreamSynchronize(h->st));
  h->check_overflow();
  CD_API_END
}

int cd_op_attention_prec(cd_handle h, const float* q, const float* k, const float* v, int B, int H, int Tq, int Tk, int D,
                         int padq, int padk, int padv, float scale, int q_log2, const float* obias, int mode, int precision,
                         void* o) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && q && k && v && o && B > 0 && H > 0 && Tq > 0 && Tk > 0 && D > 0 && padq >= 0 && padk >= 0 && padv >= 0,
           "bad argument");
  CD_CHECK(mode >= 0 && mode <= 2 && (precision == 1 || (precision == 2 && mode == 2)),
           "bad argument (mode 0 = attention_f32_fwd, 1 = one wave per query, 2 = flash; the split output is mode 2's)");
  ArenaScope arena_scope(h->arena);
  Ctx c = prec_ctx(h, precision);
  const int C = H * D;
  Act out;
  if (mode == 2) {
    CD_CHECK(!obias, "attention_flash_f32_fwd takes no output bias");
    Act qa = op_upload_rows(h, q, (int64_t)B * Tq, C, padq);
    Act ka = op_upload_rows(h, k, (int64_t)B * Tk, C, padk);
    Act va = op_upload_rows(h, v, (int64_t)B * Tk, C, padv);
    out = attention_flash_f32_fwd(c, qa.pf(), qa.ld, ka.pf(), ka.ld, (int64_t)Tk * ka.ld, va.pf(), va.ld, (int64_t)Tk * va.ld, B,
                                  H, Tq, Tk, D, scale, Tq, 1, q_log2 != 0);
  } else {
    CD_CHECK(Tq == Tk && !q_log2 && padk == 0, "modes 0 and 1 take one fused q | k tensor (Tq = Tk, its padding in padq)");
    const int T = Tq, ld = 2 * C + padq;
    float* qk = op_nan_buffer(h, (size_t)B * T * ld);
    op_put_cols(h, qk, ld, 0, q, (int64_t)B * T, C);
    op_put_cols(h, qk, ld, C, k, (int64_t)B * T, C);
    const Act va = op_upload_rows(h, v, (int64_t)B * T, C, padv);
    if (mode == 0) {
      out = attention_f32_fwd(c, op_rows_view(qk, B, T, 2 * C, ld, true), op_rows_view(va.p, B, T, C, va.ld, true), H, D, scale,
                              obias);
    } else {
      out = alloc_act(c, B, T, 1, C);
      launch_attention_f32(h->st, qk, ld, qk + C, ld, va.pf(), va.ld, out.pf(), out.ld, B, H, T, D, scale, obias);
    }
  }
  CD_CHECK(out.split == (precision == 2), "attention: output form");
  op_download(h, out, (size_t)B * Tq * C, o);
  CD_API_END
}

int cd_op_rows_prec(cd_handle h, int op, const float* x0, int64_t rows, int C0, int pad0, const float* x1, int C1, int pad1,
                    const float* gamma, const float* beta, int precision, void* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x0 && y && rows > 0 && C0 > 0 && pad0 >= 0 && pad1 >= 0, "bad argument");
  CD_CHECK(precision == 1 || precision == 2, "bad argument (precision 1 = fp32, 2 = fp32 split)");
  CD_CHECK(x1 ? (C1 > 0 && op == 2) : C1 == 0, "bad argument (second source: split_rows only)");
  ArenaScope arena_scope(h->arena);
  Ctx c = prec_ctx(h, precision);
  Act a0 = op_upload_rows(h, x0, rows, C0, pad0);
  Act out;
  if (op == 0) {
    CD_CHECK(gamma && beta, "layernorm: gain and bias");
    LNW w; w.g = const_cast<float*>(gamma); w.b = const_cast<float*>(beta); w.C = C0;
    out = layernorm_fwd(c, w, a0);
  } else if (op == 1) {
    out = geglu_f32_fwd(c, a0);
  } else if (op == 2) {
    Act a1;
    if (x1) a1 = op_upload_rows(h, x1, rows, C1, pad1);
    out = split_rows_f32_fwd(c, a0, x1 ? &a1 : nullptr);
  } else {
    CD_CHECK(false, "bad argument (op 0 = LayerNorm, 1 = GEGLU, 2 = split_rows)");
  }
  CD_CHECK(out.split == (precision == 2), "rows: output form");
  op_download(h, out, (size_t)rows * out.C, y);
  CD_API_END
}

int cd_op_resample_prec(cd_handle h, int op, const float* x, int B, int C, int H, int W, int precision, void* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && B > 0 && C > 0 && C % 4 == 0 && H > 0 && W > 0, "bad argument");
  CD_CHECK((op == 0 && (precision == 1 || precision == 2) && H % 2 == 0 && W % 2 == 0) || (op == 1 && precision == 1),
           "bad argument (op 0 = 2x2 average pool, fp32 or split; 1 = nearest x2 upsample, fp32)");
  ArenaScope arena_scope(h->arena);
  Ctx c = prec_ctx(h, precision);
  if (precision == 2) {
    Act a = op_upload_nhwc_split(h, x, B, C, C, H, W);
    Act out = avgpool2_fwd(c, a);
    CD_CHECK(out.split, "avgpool: split output expected");
    op_download(h, out, (size_t)out.rows() * C, y);
  } else {
    Act a = op_upload_nhwc(h, x, B, C, C, C, H, W);
    Act out = op == 0 ? avgpool2_fwd(c, a) : upsample2_fwd(c, a);
    op_download_nchw(h, out.p, true, out.ld, (float*)y, B, C, out.H * out.W);
  }
  CD_API_END
}

// ---- bare entry points of the small kernels of elementwise.hip: the caller's device bytes in, one launch, the kernel's bytes
// out. No staging kernel of the engine's touches either side (16-bit tensors are the storage words themselves).
static void op_bare_done(cd_handle h) {
  HIP_CHECK(hipGetLastError());  // a launch the runtime refused (its dynamic LDS, its grid) is an error, not an unchanged output
  HIP_CHECK(hipStreamSynchronize(h->st));
}

int cd_op_layout(cd_handle h, int to_nchw, const void* x, void* y, int B, int C, int HW, int ld, int src_f32, float scale,
                 float shift, int dup) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && B > 0 && C > 0 && HW > 0 && ld >= C, "bad argument");
  if (to_nchw) {
    CD_CHECK(dup == 0, "bad argument (dup: NCHW -> NHWC only)");
    launch_nhwc_to_nchw(h->st, x, src_f32 != 0, ld, (float*)y, B, C, HW, scale, shift);
  } else {
    CD_CHECK(src_f32 == 1, "bad argument (NCHW -> NHWC reads fp32)");
    launch_nchw_to_nhwc(h->st, (const float*)x, (bf16_t*)y, B, C, HW, ld, scale, shift, dup);
  }
  op_bare_done(h);
  CD_API_END
}

int cd_op_resample16(cd_handle h, int op, const void* x, void* y, int B, int H, int W, int C) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && B > 0 && H > 0 && W > 0 && C > 0 && (op == 0 || op == 1), "bad argument");
  if (op == 0) {
    CD_CHECK(H >= 2 && W >= 2, "bad argument (avgpool: H, W >= 2)");
    launch_avgpool2(h->st, (const bf16_t*)x, (bf16_t*)y, B, H, W, C);
  } else {
    launch_upsample2(h->st, (const bf16_t*)x, (bf16_t*)y, B, H, W, C);
  }
  op_bare_done(h);
  CD_API_END
}

int cd_op_copy_rows16(cd_handle h, const void* src, int lds, void* dst, int ldd, int64_t rows, int cols) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && src && dst && rows > 0 && cols > 0 && lds >= cols && ldd >= cols, "bad argument");
  launch_copy_strided_bf16(h->st, (const bf16_t*)src, lds, (bf16_t*)dst, ldd, rows, cols);
  op_bare_done(h);
  CD_API_END
}

int cd_op_vec_linear(cd_handle h, const float* x, int ldx, const float* W, const float* bias, float* y, int ldy, int B, int K,
                     int N, int silu_in, int silu_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && W && y && B > 0 && K > 0 && N > 0 && ldx >= K && ldy >= N, "bad argument");
  launch_vec_linear(h->st, x, ldx, W, bias, y, ldy, B, K, N, silu_in, silu_out);
  op_bare_done(h);
  CD_API_END
}

int cd_op_tokens(cd_handle h, int op, const int* ids, const void* x16, const float* tok, const float* pos, void* out, int B,
                 int L, int D, int vocab) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && out && B > 0 && L > 0 && D > 0, "bad argument");
  if (op == 0) {
    CD_CHECK(ids && tok && pos && vocab > 0, "bad argument (embed_tokens: ids, table, positions)");
    launch_embed_tokens(h->st, ids, tok, pos, (bf16_t*)out, B, L, D, vocab);
  } else if (op == 1) {
    CD_CHECK(x16 && tok && pos, "bad argument (vit_tokens: patches, class row, positions)");
    launch_vit_tokens(h->st, (const bf16_t*)x16, tok, pos, (bf16_t*)out, B, L, D);
  } else if (op == 2) {
    CD_CHECK(x16 && ids, "bad argument (gather_eot: rows, ids)");
    launch_gather_eot(h->st, (const bf16_t*)x16, ids, (bf16_t*)out, B, L, D);
  } else {
    CD_CHECK(false, "bad argument (op 0 = embed_tokens, 1 = vit_tokens, 2 = gather_eot)");
  }
  op_bare_done(h);
  CD_API_END
}

int cd_op_posterior_sample(cd_handle h, const float* mom, int ld, const float* noise, uint64_t seed, float* z, int B, int zc,
                           int HW, float scale, int use_mean) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && mom && z && B > 0 && zc > 0 && HW > 0 && ld >= 2 * zc, "bad argument");
  launch_posterior_sample(h->st, mom, ld, noise, seed, z, B, zc, HW, scale, use_mean);
  op_bare_done(h);
  CD_API_END
}

int cd_op_vq_quantize(cd_handle h, const float* z, float in_mul, const float* codebook, int n_embed, int zc, int B, int HW,
                      void* out16, int Cpad) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && z && codebook && out16 && B > 0 && HW > 0 && Cpad >= zc, "bad argument");
  launch_vq_quantize(h->st, z, in_mul, codebook, n_embed, zc, B, HW, (bf16_t*)out16, Cpad);
  op_bare_done(h);
  CD_API_END
}

// ---- the implicit-GEMM kernel as the batched plain GEMM of the V^T / S = QK^T / O = PV call sites, on the caller's bytes:
// one launch_conv_gemm whose parameters are filled the way those sites fill them (the launcher's own checks refuse a bad call)
int cd_op_gemm_batched(cd_handle h, const void* a, int lda, int64_t a_bs, const void* w, int ldw, int64_t w_bs, int M, int N,
                       int K, int nbatch, float alpha, const float* bias, const void* resid, int resid_ld, float* stats, int act,
                       int tile, void* out, int out_ld, int64_t o_bs, int out_f32) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && a && w && out && M > 0 && N > 0 && K > 0 && nbatch > 0 && lda > 0 && ldw > 0 && out_ld > 0, "bad argument");
  Ctx c = h->ctx();
  ConvGemmParams p;
  p.src0 = (const bf16_t*)a; p.C0 = K; p.ld0 = lda;
  p.B = 1; p.Hs = M; p.Ws = 1; p.Hin = M; p.Win = 1; p.Hout = M; p.Wout = 1;
  p.M = M;
  p.wgt = (const bf16_t*)w; p.Ktot = K; p.ldw = ldw; p.N = N;
  p.nbatch = nbatch; p.a_bs = a_bs; p.w_bs = w_bs; p.o_bs = o_bs;
  p.alpha = alpha; p.bias = bias; p.resid = (const bf16_t*)resid; p.resid_ld = resid_ld; p.stats = stats; p.act = act;
  p.tile = tile;
  p.out = out; p.out_ld = out_ld; p.out_f32 = out_f32; p.zeros = c.zeros;
  launch_conv_gemm(h->st, p);
  op_bare_done(h);
  CD_API_END
}

// at_core (engine.hip) with one head on the caller's q | k rows, normalised rows and output; vt_out (or NULL) receives V^T
// [B][C][Tpad]
int cd_op_attn_block_core(cd_handle h, const void* qk, int ldqk, const void* n, int ldn, const void* packed_v,
                          const float* v_bias, int B, int T, int C, void* o, int ldo, void* vt_out, int* branch) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && qk && n && packed_v && o && B > 0 && T > 0 && C > 0 && ldqk >= 2 * C && ldn >= C && ldo >= C, "bad argument");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  const ConvW& wv = *(const ConvW*)packed_v;
  CD_CHECK(wv.N == C && wv.Cpad == C && wv.KH == 1 && wv.KW == 1, "packed weight does not match the call");
  const AtCoreOut r = at_core(c, wv, v_bias, op_rows_view(qk, B, T, 2 * C, ldqk, false), op_rows_view(n, B, T, C, ldn, false), C,
                              /*heads=*/1, op_rows_view(o, B, T, C, ldo, false));
  if (vt_out) HIP_CHECK(hipMemcpyAsync(vt_out, r.vt, (size_t)B * C * r.Tpad * 2, hipMemcpyDeviceToDevice, h->st));
  if (branch) *branch = r.branch;
  op_bare_done(h);
  CD_API_END
}

// ---- the FID Inception-v3's own kernels and launch forms (inception.hip), through the launchers the network calls
int cd_op_pool3x3(cd_handle h, const float* x, int B, int C, int H, int W, int in_pad, int max, int stride, int pad,
                  int out_off, int out_ld, float* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && B > 0 && C > 0 && H > 0 && W > 0 && stride > 0 && pad >= 0 && in_pad >= 0 && out_off >= 0, "bad argument");
  CD_CHECK(C % 8 == 0 && in_pad % 8 == 0 && out_off % 8 == 0 && out_ld % 8 == 0, "C, in_pad, out_off, out_ld: multiples of 8 elements");
  CD_CHECK(out_off + C <= out_ld, "the slice [%d, %d) does not fit a row of %d", out_off, out_off + C, out_ld);
  CD_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3, "bad argument (image smaller than the window)");
  ArenaScope arena_scope(h->arena);
  const Act a = op_upload_nhwc16(h, x, B, C, C + in_pad, H, W);
  const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
  const int64_t rows = (int64_t)B * Ho * Wo;
  bf16_t* ob = op_nan_rows16(h, rows, out_ld);
  launch_pool3x3(h->st, a.p, a.ld, B, H, W, C, max != 0, stride, pad, ob + out_off, out_ld);
  op_download_nchw(h, ob, false, out_ld, y, (int)rows + 64, out_ld, 1);
  CD_API_END
}

int cd_op_global_avg(cd_handle h, const float* x, int B, int HW, int C, int in_pad, float* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && B > 0 && HW > 0 && C > 0 && in_pad >= 0, "bad argument");
  CD_CHECK(C % 8 == 0 && in_pad % 8 == 0, "C, in_pad: multiples of 8 elements");
  ArenaScope arena_scope(h->arena);
  const Act a = op_upload_nhwc16(h, x, B, C, C + in_pad, HW, 1);
  launch_global_avg(h->st, a.p, a.ld, B, HW, C, y);
  CD_API_END
}

int cd_op_basic_conv(cd_handle h, const float* x, int B, int Cin, int H, int W, int in_ld, const float* w, const float* gamma,
                     const float* beta, const float* mean, const float* var, int N, int KH, int KW, int stride, int pad_t,
                     int pad_l, int out_off, int out_ld, int tile, float* y, float* w_packed, float* bias_out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && w && gamma && beta && mean && var && y, "bad argument");
  CD_CHECK(B > 0 && Cin > 0 && H > 0 && W > 0 && N > 0 && KH > 0 && KW > 0 && stride > 0 && pad_t >= 0 && pad_l >= 0 &&
               out_off >= 0, "bad argument");
  CD_CHECK(H + 2 * pad_t >= KH && W + 2 * pad_l >= KW, "bad argument (image smaller than the filter)");
  const int Cpad = round_up(Cin, 32), Nrun = round_up(N, 32);
  CD_CHECK(in_ld % 8 == 0 && in_ld >= Cpad, "in_ld: a multiple of 8 elements, at least round_up(Cin, 32) = %d", Cpad);
  CD_CHECK(out_off % 8 == 0 && out_ld % 8 == 0, "out_off, out_ld: multiples of 8 elements");
  CD_CHECK(out_off + Nrun <= out_ld, "the slice [%d, %d) does not fit a row of %d", out_off, out_off + Nrun, out_ld);
  ConvW* cw = h->op_params.new_conv(N, Cin, KH, KW, true);  // as InceptionFID::unit: zeroed [Npad][KH][KW][Cpad] and bias [Npad]
  CD_CHECK(cw->Cpad == Cpad, "basic_conv: channel padding");
  ArenaScope arena_scope(h->arena);
  Ctx c = h->ctx();
  launch_fold_bn(h->st, w, gamma, beta, mean, var, N, Cin, KH, KW, Cpad, cw->w, cw->b);
  const Act a = op_upload_nhwc16(h, x, B, Cin, in_ld, H, W, Cpad);
  const int Ho = (H + 2 * pad_t - KH) / stride + 1, Wo = (W + 2 * pad_l - KW) / stride + 1;
  const int64_t rows = (int64_t)B * Ho * Wo;
  bf16_t* ob = op_nan_rows16(h, rows, out_ld);
  ConvGemmParams p = basic_conv_params(a.p, a.ld, B, H, W, Cpad, cw->w, cw->b, N, KH, KW, stride, pad_t, pad_l, ob + out_off,
                                       out_ld, c.zeros);
  CD_CHECK(p.M == rows && p.N == Nrun, "basic_conv: geometry");
  p.tile = tile;
  launch_conv_gemm(h->st, p);
  op_download_nchw(h, ob, false, out_ld, y, (int)rows + 64, out_ld, 1);
  if (w_packed) op_download_nchw(h, cw->w, false, cw->Ktot(), w_packed, cw->Npad, cw->Ktot(), 1);
  if (bias_out) HIP_CHECK(hipMemcpyAsync(bias_out, cw->b, (size_t)cw->Npad * sizeof(float), hipMemcpyDeviceToDevice, h->st));
  CD_API_END
}

// ---- the LPIPS kernels (lpips.hip), through the launchers the network calls
int cd_op_lpips_layer(cd_handle h, const float* f0, const float* f1, const float* w, int B, int HW, int C, int in_pad,
                      float* out) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && f0 && f1 && w && out && B > 0 && HW > 0 && C > 0 && in_pad >= 0, "bad argument");
  CD_CHECK((int64_t)B * HW < (1 << 30), "bad argument (too many rows)");
  ArenaScope arena_scope(h->arena);
  const int ld = C + in_pad;
  const int64_t rows = (int64_t)B * HW;
  float* part = (float*)h->arena.alloc((size_t)B * lpips_layer_chunks(HW, C > 512 ? 512 : C) * sizeof(float));
  if (C % 8 == 0 && C <= 512 && ld % 8 == 0) {  // else: the launcher refuses below, before anything is staged
    bf16_t* a = op_nan_rows16(h, rows, ld);
    bf16_t* b = op_nan_rows16(h, rows, ld);
    op_put_cols16(h, a, ld, 0, f0, rows, C);
    op_put_cols16(h, b, ld, 0, f1, rows, C);
    launch_lpips_layer(h->st, a, b, ld, B, HW, C, w, part, nullptr, 0, false, out);
  } else {
    launch_lpips_layer(h->st, nullptr, nullptr, ld, B, HW, C, w, part, nullptr, 0, false, out);
  }
  CD_API_END
}

int cd_op_pool2x2(cd_handle h, const float* x, int B, int C, int H, int W, int in_pad, int out_off, int out_ld, float* y) {
  CD_API_BEGIN
  enter_engine(h);
  CD_CHECK(h && x && y && B > 0 && C > 0 && H > 0 && W > 0 && in_pad >= 0 && out_off >= 0, "bad argument");
  CD_CHECK(C % 8 == 0 && in_pad % 8 == 0 && out_off % 8 == 0 && out_ld % 8 == 0, "C, in_pad, out_off, out_ld: multiples of 8 elements");
  CD_CHECK(out_off + C <= out_ld, "the slice [%d, %d) does not fit a row of %d", out_off, out_off + C, out_ld);
  CD_CHECK(H >= 2 && W >= 2, "bad argument (image smaller than the window)");
  ArenaScope arena_scope(h->arena);
  const Act a = op_upload_nhwc16(h, x, B, C, C + in_pad, H, W);
  const int64_t rows = (int64_t)B * (H / 2) * (W / 2);
  bf16_t* ob = op_nan_rows16(h, rows, out_ld);
  launch_pool2x2(h->st, a.p, a.ld, B, H, W, C, ob + out_off, out_ld);
  op_download_nchw(h, ob, false, out_ld, y, (int)rows + 64, out_ld, 1);
  CD_API_END
}

}  // extern "C"

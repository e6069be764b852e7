// Launcher declarations for the hand-written gfx950 kernels (implementation: *.hip in this dir).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace cd {

// ---------------------------------------------------------------- scheduler (sched.hip)
// Per-step scalar coefficients, evaluated on the host in fp32 in the reference's operation
// order (ddim.py:570-579). DDIM-eta form:
//   sa=sqrt(a_t) s1a=sqrt(1-a_t) sap=sqrt(a_prev) dirc=sqrt(1-a_prev-sigma^2) sigma r=sqrt(1-a_t)
// DDPM form (pixel 'ddpm'): see sched.hip k_encode_step_ddpm.
struct StepCoef {
  float sa, s1a, sap, dirc, sigma, r, t_mask;
  int t;  // integer timestep fed to the U-Net
};
enum { SCHED_DDIM = 0, SCHED_DDPM = 1 };

struct EpsHat {  // network output view: element (b,c,p) at p[b*sb + c*sc + p*sp]
  const float* p = nullptr;
  int64_t sb = 0, sc = 0, sp = 0;
  int cfg = 0;   // 1: batch is [uncond B | cond B], combine with guidance scale g
  float g = 1.f;
  const float* gvec = nullptr;  // per-sample guidance scales [B] (device) instead of g: ensemble members that differ only
                                // in their decoder scale share one launch set
};

// Arguments of the step kernels, passed to them by value; every default means "off".
struct StepGeom {  // the batch and this step's row of the device-resident coefficient table
  int B = 0, C = 0, HW = 0;
  const StepCoef* tab = nullptr;
  int step = 0;
};
struct GaussSrc {  // a standard-normal draw per element: the tensor [B, C, HW], or null -> Philox(seed, stream)
  const float* noise = nullptr;
  uint64_t seed = 0;
  uint32_t stream = 0;
};
struct XinOut {  // the next forward's 16-bit NHWC input [B, HW, cpad], or null -> not written
  bf16_t* xin = nullptr;
  int cpad = 0;
  int dup = 0;  // n: written n more times, each B samples on (1: the classifier-free-guidance batch [uncond | cond] of one
                // x_t; 1 + E: semantic guidance's [uncond | E concepts | cond] - the step kernels of sched.hip only: the
                // ILVR and keep-mask-estimate kernels take 0 / 1)
};
struct EpsIn {  // injected eps (decode only): sample b at p[b * bstride], or null -> drawn from the GaussSrc
  const float* p = nullptr;
  int64_t bstride = 0;
  int bmod = 0;  // > 0: sample b takes the eps of sample b % bmod (the coupled loop decodes several guidance scales of the
                 // same bmod encoder samples in one batch)
};
struct ZSlot {  // where init / encode store x_T / eps (sample b at p[b * bstride]); init: null -> not stored
  float* p = nullptr;
  int64_t bstride = 0;
};
struct StepArgs {
  const float* x0 = nullptr;  // init / encode: the clean sample
  float* xt = nullptr;        // the running latent, updated in place
  EpsHat eh;                  // encode / decode
  StepGeom geom;
  GaussSrc gauss;
  XinOut xin;
  EpsIn eps;       // decode
  ZSlot z;         // init / encode
  int is_last = 0; // encode ('ddim'): x_next = x0 without a draw
};

// region-keeping decode (ddim.py:427-430): what the masked step kernels blend into the decoder's latent ahead of a forward
struct MaskBlend {
  const float* mask = nullptr;   // [mask_bmod, 1, HW], 1 = keep the source
  const float* src = nullptr;    // "q_sample": x0 [src_bmod, C, HW]; "encoder": the DPM-Encoder's x_t [src_bmod, C, HW]
  int mask_bmod = 1, src_bmod = 1;
  const float2* qtab = nullptr;  // "q_sample": (sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod)[tau[k]] by row k; else null
  int qrow = 0;                  // row of the level being blended
  GaussSrc gauss;                // "q_sample": that level's draw
};

void launch_init_xt(hipStream_t st, const StepArgs& a);
void launch_encode_step(hipStream_t st, int kind, const StepArgs& a);
// mk: SCHED_DDIM only, the step is followed by the blend of the next level unless blend is false (the keep-mask entry points'
// last step; the local blend of DESIGN.md 18 blends after every step, the last included)
void launch_decode_step(hipStream_t st, int kind, const StepArgs& a, const MaskBlend* mk = nullptr, bool blend = false);
// a.xt <- blend(a.xt) ahead of the first forward; uses a.geom and a.xin beside it
void launch_mask_blend_init(hipStream_t st, const StepArgs& a, const MaskBlend& mk);
// out[i] = the draw of element first + i from g, i < n (cd_op_gauss: the generator as the tests see it)
void launch_gauss_fill(hipStream_t st, GaussSrc g, int64_t first, float* out, int64_t n);

// ---------------------------------------------------------------- semantic guidance (sega.hip)
constexpr int kSegaMaxConcepts = 8;
struct SegaConcept {  // == cd_sega_concept: one edit concept, its threshold as the two order statistics' rank and weight
  float scale, weight;  // s_e (signed: negative steers away), w_e
  int lo;               // floor(q * (N - 1))
  float frac;           // q * (N - 1) - lo, in [0, 1)
  int warm, cool;       // active on iterations warm <= i < cool
};
// One iteration's guidance on the Bd decoder rows. eh views the network's output from the decoder's first row on: batch rows
// [uncond Bd | concept 0 Bd | ... | concept E-1 Bd | cond Bd]; eh.g / eh.gvec the row's guidance scale (eh.cfg is not read).
struct SegaStep {
  EpsHat eh;
  int Bd = 0, C = 0, HW = 0, E = 0;
  uint32_t active = 0;               // bit e: concept e is active in this iteration
  const SegaConcept* tab = nullptr;  // [E], device
  float* abuf = nullptr;             // [Bd * E, C * HW] scratch: |d_e| of the active concepts
  float* tau = nullptr;              // [Bd, E], written for the active concepts only
  int* kept = nullptr;               // [Bd, E], #{a >= tau}, likewise
  float* nu = nullptr;               // [Bd, C, HW] momentum, in / out
  float* eps = nullptr;              // [Bd, C, HW] fp32 NCHW: what the decode step reads through an EpsHat with cfg = 0
  float* mask_out = nullptr;         // [Bd, E, C, HW] of 0 / 1 (0 for an inactive concept), or null
  float s_m = 0.f, beta = 0.f;
};
// k_sega_threshold on a (Bd, active concepts) grid - not launched when none is active - then k_sega_combine
void launch_sega_guidance(hipStream_t st, const SegaStep& a);

// ---------------------------------------------------------------- ILVR low-pass conditioning (ilvr.hip)
// A resize matrix M [n_out, n_in] as its nonzero taps: row i is w[t * n_out + i] at column first[i] + t, t = 0 .. P-1
// (tap-major, so that neighbouring lanes read neighbouring rows). The host has folded the mirrored border taps into the
// interior and clamped first[i] to [0, n_in - P]: a kernel never tests a boundary.
struct LowpassTaps {
  const float* w = nullptr;
  const int* first = nullptr;
  int n_out = 0, n_in = 0, P = 0;
};
// x <- x' + phi_N(y' - x'), phi_N(X) = U D X D^T U^T per channel image, y' = qa * y + qb * n; two launches:
//   launch_ilvr_down    T[b, c] = D (y' - x') D^T   [B, C, r, r], r = R / N
//   launch_ilvr_up_add  out = x' + U T U^T          (and the next forward's 16-bit input, if xin is set)
// Fixed summation order: taps ascending (compensated), the row index of the image first, then the column index.
struct IlvrArgs {
  const float* xp = nullptr;     // x' [B, C, R, R]; null = 0 (cd_op_lowpass)
  float* out = nullptr;          // [B, C, R, R]; may be xp
  const float* y = nullptr;      // the reference image [y_bmod, C, R, R]: sample b reads row b % y_bmod
  int y_bmod = 1;
  const float2* qtab = nullptr;  // (qa, qb) by row; null = (1, 0)
  int qrow = 0;
  GaussSrc gauss;                // n; not drawn when qb == 0
  float* T = nullptr;
  int B = 0, C = 0, R = 0;
  LowpassTaps D, U;              // D [r, R], U [R, r]
  XinOut xin;
  int vec4 = 0;                  // 1: R % 4 == 0 and every tensor is 16-byte aligned
};
constexpr int kIlvrMaxR = 1024;
// resize_matrix(n_in, n_out) of utils/lowpass.py as taps, in float64 on the host, rounded once: w [P][n_out], first [n_out]
void build_lowpass_taps(int n_in, int n_out, std::vector<float>& w, std::vector<int>& first, int& P);
void launch_ilvr_down(hipStream_t st, const IlvrArgs& a);
void launch_ilvr_up_add(hipStream_t st, const IlvrArgs& a);

// ---------------------------------------------------------------- keep-mask estimation (automask.hip)
// x_i = qa*x0 + qb*n_i for n_draws draws of one forward: rows (i, b) of its input, i-major
struct AutoMaskNoised {
  const float* x0 = nullptr;     // [B, C, HW]
  float qa = 1.f, qb = 0.f;
  const float* noise = nullptr;  // [n_draws, B, C, HW], or null -> Philox(seed, stream0 + i), element = the flat index in [B, C, HW]
  uint64_t seed = 0;
  uint32_t stream0 = 0;
  int n_draws = 0, B = 0, C = 0, HW = 0;
  XinOut xin;                    // 16-bit NHWC [n_draws * B (twice with dup), HW, cpad], or null
  float* xq = nullptr;           // fp32 NCHW [n_draws * B, C, HW], or null
};
constexpr int kAutoMaskMaxDilate = 8;
struct AutoMaskArgs {
  // accumulate: element (i, b, c, p) of either prediction at [(i * B + b) * sb + c * sc + p * sp]
  const float* e_src = nullptr;
  const float* e_tgt = nullptr;
  int64_t sb = 0, sc = 0, sp = 0;
  int n_chunk = 0;         // draws in this launch
  int first = 0;           // 1: acc starts from 0, else from what lies there
  float* acc = nullptr;    // [B, HW]: sum over draws and channels of |e_tgt - e_src|
  int B = 0, C = 0, H = 0, W = 0;
  // finish: map = acc / float(n_total * C)
  int n_total = 0;
  float ratio = 3.f, thr = 0.5f;
  int dilate = 0;
  float* partial = nullptr;   // [B, nblk] block sums of map, nblk = automask_sum_blocks(H * W)
  int nblk = 0;
  float* map_out = nullptr;   // [B, HW] or null
  float* mean_out = nullptr;  // [B] or null
  float* keep_out = nullptr;  // [B, HW], exact 0 / 1 (1 = keep the source)
};
int automask_sum_blocks(int HW);
void launch_automask_qsample(hipStream_t st, const AutoMaskNoised& a);
void launch_automask_accum(hipStream_t st, const AutoMaskArgs& a);
void launch_automask_finish(hipStream_t st, const AutoMaskArgs& a);  // the per-image sum, then threshold / dilation / output

// ---------------------------------------------------------------- per-word attention maps (automask.hip)
// One included layer of a forward into that forward's per-row sums: acc[r][n][y][x] (+)= layer[r][n][(y / f) * s + x / f],
// f = h / s. A row is (draw i, sample b) = i * B + b, so a draw's layers add up in the forward's order whichever forward
// the draw runs in.
struct WordMapAccum {
  const float* layer = nullptr;  // [rows][N][s * s]
  float* acc = nullptr;          // [rows][N][h][w]
  int rows = 0, N = 0, s = 0, h = 0, w = 0;
  int first = 0;                 // 1: acc starts from 0, else from what lies there
};
void launch_word_map_accumulate(hipStream_t st, const WordMapAccum& a);
// The draws of one forward into the call's sums, ascending: total[b][e] (+)= acc[0 * B + b][e] + ... ; with `out`,
// out = total * scale afterwards (the last forward of a call).
struct WordMapFold {
  const float* acc = nullptr;  // [n_chunk * B][per]
  float* total = nullptr;      // [B][per]
  float* out = nullptr;        // [B][per] or null
  int n_chunk = 0, B = 0;
  int64_t per = 0;             // N * h * w
  int first = 0;               // 1: total starts from 0
  float scale = 1.f;
};
void launch_word_map_fold(hipStream_t st, const WordMapFold& a);

// ---------------------------------------------------------------- prompt-to-prompt local blend (automask.hip)
// The keep-mask of one decoder row from the running sums of the word maps: for A = acc_src[r % B] and A = acc_tgt[r],
//   p = max of A over |dy|, |dx| <= pool / 2 inside the image, mx = max p, e_A = mx > 0 && p / mx > thr;
//   keep[r][y][x] = 1 - (e_src | e_tgt) at cell (y / f, x / f): exact 0 / 1 on the [side * f]^2 latent grid.
constexpr int kBlendMaxSide = 64;  // both maps of a row stay in LDS: 2 * 64 * 64 * 4 B
constexpr int kBlendMaxPool = 7;
struct LocalBlendMask {
  const float* acc_src = nullptr;  // [B][side][side]
  const float* acc_tgt = nullptr;  // [Bd][side][side]
  float* keep = nullptr;           // [Bd][side * f][side * f]
  int B = 0, Bd = 0, side = 0, f = 1, pool = 1;
  float thr = 0.f;
};
void launch_local_blend_mask(hipStream_t st, const LocalBlendMask& a);

// ---------------------------------------------------------------- fused windows (windows.hip)
// The latent lives on a canvas [Hc, Wc] >= the network's S x S; window w is the S x S crop at win[w] = (y_w, x_w), inside the
// canvas (the callers check it on the host). Network rows are window-major inside a part: row d * n_win * Bp + w * Bp + b.
constexpr int kMaxWindows = 64;
struct WindowGather {  // y[d][w][b][S * S][cpad] 16-bit NHWC <- x[b][:, y_w : y_w + S, x_w : x_w + S], channels C.. zero
  const float* x = nullptr;  // [Bp][C][Hc][Wc] fp32
  bf16_t* y = nullptr;       // (1 + dup) parts, every part the same values (the [uncond | cond] rows of one latent)
  const int* win = nullptr;  // [n_win][2] device
  int Bp = 0, C = 0, Hc = 0, Wc = 0, S = 0, n_win = 0, cpad = 0, dup = 0;
};
void launch_window_gather(hipStream_t st, const WindowGather& a);
// out[d * Bp + b][c][y][x] = (e_{w_first} + e_w + ...) / (float)count over the windows covering (y, x), ascending w, fp32, no
// contraction; acc starts from the first covering value, so one covering window returns its value bit for bit
struct WindowFuse {
  const float* e = nullptr;  // [parts][n_win][Bp][S * S][ld] fp32, the first C of ld channels are read
  float* out = nullptr;      // [parts * Bp][C][Hc][Wc] fp32
  const int* win = nullptr;  // [n_win][2] device
  int Bp = 0, C = 0, Hc = 0, Wc = 0, S = 0, n_win = 0, ld = 0, parts = 1;
};
void launch_window_fuse(hipStream_t st, const WindowFuse& a);

// ---------------------------------------------------------------- implicit-GEMM conv / GEMM (conv_gemm.hip)
enum { ACT_NONE = 0, ACT_SILU = 1, ACT_GELU = 2, ACT_GEGLU = 3, ACT_QGELU = 4, ACT_RELU = 5 };  // QGELU: x*sigmoid(1.702x) (CLIP)
// RELU: max(x, 0) (the BasicConv2d units of the FID Inception-v3, inception.hip)

struct ConvGemmParams {
  // A operand: activations, NHWC bf16; optional second source = channel concat (th.cat, openaimodel.py:736)
  const bf16_t* src0 = nullptr;
  const bf16_t* src1 = nullptr;
  int C0 = 0, C1 = 0;        // channels taken from each source (multiples of 32)
  int ld0 = 0, ld1 = 0;      // pixel stride in elements
  int B = 1, Hs = 1, Ws = 1; // stored spatial dims of the sources
  int up = 0;                // 1: nearest x2 upsample folded into the gather (F.interpolate, openaimodel.py:115)
  int Hin = 1, Win = 1;      // logical input dims (= 2*Hs when up)
  int KH = 1, KW = 1, stride = 1, pad_t = 0, pad_l = 0;
  int Hout = 1, Wout = 1;
  int M = 0;                 // B*Hout*Wout
  // B operand: weights [Npad][Ktot] bf16, k = (r*KW+s)*(C0+C1) + c
  const bf16_t* wgt = nullptr;
  const bf16_t* wgt_frag = nullptr;  // the same weights in MFMA-fragment-major order (lin_stream.hip), or null
  int Ktot = 0, N = 0;
  int ldw = 0;               // weight row stride in elements (0 = Ktot)
  // batched GEMM (grid.z): element strides
  int nbatch = 1;
  int64_t a_bs = 0, w_bs = 0, o_bs = 0;
  // epilogue: out = act(alpha*acc + bias[n] + rowvec[m/rows_per_vec][n]) + resid[m][n]
  float alpha = 1.0f;
  const float* bias = nullptr;
  const float* rowvec = nullptr;
  int rowvec_ld = 0, rows_per_vec = 1;
  const bf16_t* resid = nullptr;
  int resid_ld = 0;
  int resid_f32 = 0;         // the residual is fp32 (the split-fp16 mode of the fp32 path, f32_path.hip)
  int act = ACT_NONE;
  void* out = nullptr;
  int out_ld = 0;
  int out_f32 = 0;
  // optional fused GroupNorm statistics of the output: [nbatch][ceil(M/32)][2][N] fp32 (sum | sum of squares
  // per channel over each 32-row block); null = off. Not available with GEGLU.
  float* stats = nullptr;
  const bf16_t* zeros = nullptr;  // >= 256 B of zeros (masked rows / padding taps)
  // the rows of A are LayerNorm-ed (no gain / bias: those are folded into wgt / bias) inside the kernel; lin_stream only
  int ln_fold = 0;
  float ln_eps = 1e-5f;
  int tile = 0;                   // 0 = auto (tile configuration AND split factor from the autotuner)
  float prof_flop_scale = 1.f;    // KernelProfiler books 2*M*N*Ktot times this (1/3 for the three-term split GEMMs)
  // split-K (deep-K layers whose output tiles cannot fill 256 CUs): K is cut in `splitk` ranges, fp32
  // partial tiles meet in sk_scratch and the last arrival sums them in split order. 0/1 = off.
  int splitk = 0;
  float* sk_scratch = nullptr;    // defaults to g_conv_splitk when splitk > 1
  int* sk_flags = nullptr;
  // order of the K steps of a KH x KW > 1 convolution: tap-major (all channels of a filter tap, then the next tap) or
  // channel-major (the KH * KW taps of one BK-channel slice, then the next slice: the re-reads of an activation line by
  // neighbouring taps follow each other within KH * KW steps and hit the XCD's L2 - round 4: hit rate 54 -> 72 %, fabric fetch
  // of the 320-channel 3 x 3 conv at 64 x 64 750 -> 409 MB per launch). 1 (default) = channel-major where the activation is
  // large (launch_cfg), 2 = wherever the kernel supports it, 0 = never (CYCLEDIFF_KORDER for A/B runs)
  int korder = 1;
  // tile walk inside an XCD's contiguous range: 0 = row-major in the operand the launcher picked (m-major / n-major);
  // G > 0 = groups of G row tiles walked m-fastest (the 32 CUs of an XCD then run G row tiles x 32 / G column tiles at a time:
  // G A panels + 32 / G W panels in its L2 instead of 1 + 32) - for the wide-N layers whose operands both exceed the L2
  int tile_group = 0;
  // 1: the nearest-x2 3 x 3 convolution in its phase form. After the x2 replication only 2 x 2 stored
  // pixels feed an output pixel, so the taps that share one are summed ahead of time (launch_up_phase_weights): four 2 x 2
  // convs on the stored grid, one per output parity (a, b), K = 4 C instead of 9 C. GEMM row m = (image, phase = 2 a + b,
  // y, x) with Hout = Hs, Wout = Ws, M = 4 B Hs Ws, KH = KW = 2, up = 0; the taps of row m start at (y + a - 1, x + b - 1)
  // and its weights at wgt + phase * w_ps. Hs * Ws is a multiple of 256, so a tile of any configuration lies in one phase
  // of one image. Rows leave in this order (launch_up_phase_reorder puts them in place); an image's rows, and so the
  // 32-row statistics blocks its GroupNorm sums, stay contiguous. Tap-major K order only.
  int up_phase = 0;
  int w_ps = 0;  // element stride between the four phase matrices
};
struct SplitKWorkspace {
  float* scratch = nullptr;
  size_t scratch_bytes = 0;
  int* flags = nullptr;  // zero-initialised arrival counters, one per output tile
  int nflags = 0;
};
extern thread_local SplitKWorkspace g_conv_splitk;  // the calling thread's engine (capi.hip enter_engine)
void launch_conv_gemm(hipStream_t st, const ConvGemmParams& p);
const char* conv_gemm_last_config();
// what the calling thread's most recent launch_conv_gemm ran, after every fallback (read-only; no effect on any launch)
struct GemmLaunchInfo {
  int tile_id = 0;     // the kCfgs id whose instantiation was launched (or kLinStreamTile)
  int bk = 0;          // K-step depth of that instantiation: 32 or 64
  int splitk = 1;      // effective split (1 = none)
  int chm = 0;         // 1 = the channel-major K order was taken
  int tile_group = 0;  // group size of the tile walk (0 = row-major)
};
GemmLaunchInfo conv_gemm_last_launch();
// the four phase matrices of a packed 3 x 3 weight (ConvGemmParams::up_phase): w [Npad][3][3][Cpad] -> out [2 a + b][Npad][2][2][Cpad],
// row taps {w0, w1 + w2} for a = 0 and {w0 + w1, w2} for a = 1 (columns alike with b); summed in fp32, rounded once
void launch_up_phase_weights(hipStream_t st, const bf16_t* w, bf16_t* out, int Npad, int Cpad);
int conv_gemm_num_configs();
const char* conv_gemm_config_name(int id);

// ---------------------------------------------------------------- streaming linear layer, K = 320 (lin_stream.hip)
// out[M][N] = epi(A[M][320] . W[N][320]^T): A strips resident in registers and prefetched a strip ahead, W streamed
// through LDS in fragment-major order, persistent workgroups. Part of the implicit-GEMM family: launch_conv_gemm
// dispatches to it (tile id kLinStreamTile) for the shapes lin_stream_supports() accepts.
struct LinStreamParams {
  const bf16_t* a = nullptr; int lda = 0;
  const bf16_t* wfrag = nullptr;
  const float* bias = nullptr;
  const bf16_t* resid = nullptr; int ldr = 0;
  bf16_t* out = nullptr; int ldo = 0;
  float* stats = nullptr;
  int M = 0, N = 0;
  float ln_eps = 1e-5f;  // LayerNorm-folded variants
  // V^T variants (the q | k | v projection of the 64 x 64 transformer blocks): packed columns [nsplit, N) leave
  // untransposed into vt[row / hw][column - nsplit][vt_ld], token row % hw; nsplit % 64 == 0, hw % 256 == 0
  int nsplit = 0, hw = 0;
  bf16_t* vt = nullptr; int vt_ld = 0;
  int64_t vt_bytes = 0;
  // GroupNorm-applying variant (proj_in): a = pack(a * coef[row / hw][0][k] + coef[row / hw][1][k]) ahead of the product
  const float* gn_coef = nullptr;
};
constexpr int kLinStreamTile = 30;
bool lin_stream_supports(const ConvGemmParams& p);
void launch_lin_stream(hipStream_t st, const ConvGemmParams& p);
// The entry of a 64 x 64 transformer block on the streaming kernel. Both need whole images in every 256-row strip
// (hw % 256 == 0) and 32-bit byte offsets: lin_stream_entry_supports().
bool lin_stream_entry_supports(int64_t M, int hw, int lda);
// qk[M][640] = a . W[0:640]^T + bias, vt[M / hw][320][vt_ld] = (a . W[640:960]^T + bias)^T per image; wfrag = the 960 rows
// fragment-major, bias = 960 floats or null. ln_fold: the rows of a are LayerNorm-ed in registers (statistics only)
void launch_lin_stream_qkv(hipStream_t st, const bf16_t* a, int lda, int M, int hw, const bf16_t* wfrag, const float* bias,
                           bf16_t* qk, bf16_t* vt, int vt_ld, bool ln_fold, float ln_eps);
// out[M][320] = pack(a * al + be) . W^T + bias with the per-image GroupNorm coefficients gn_coef[M / hw][2][320]
void launch_lin_stream_gn(hipStream_t st, const bf16_t* a, int lda, int M, int hw, const float* gn_coef, const bf16_t* wfrag,
                          const float* bias, bf16_t* out, int ldo);
// w_out = w . diag(gamma) (16-bit), bias_out = bias + w . beta (fp32): the weights of a LayerNorm-folded layer
void launch_fold_ln(hipStream_t st, const bf16_t* w, int ldw, const float* gamma, const float* beta, const float* bias,
                    bf16_t* w_out, float* bias_out, int N, int Kc);
// standard packed rows [N][ldw] (K = 320 used) -> fragment-major blocks [N / 32][20][64][8]
void launch_pack_wfrag(hipStream_t st, const bf16_t* w, int ldw, bf16_t* out, int N);

// Optional per-launch timing of the dominant kernel family with HIP events recorded on the launch
// stream (bench.py's roofline leg). flops = 2*M*N*K per launch (algorithmic, padding excluded except
// the 3/4 -> 32 input-channel pad of conv_in).
struct KernelProfiler {
  bool enabled = false;
  std::vector<hipEvent_t> events;
  std::vector<double> flops;
  std::vector<std::string> labels;
  int used = 0;
  bool verbose = false;  // CYCLEDIFF_GEMM_LOG=1: collect() prints a per-shape table to stderr
  struct Entry { int n = 0; double ms = 0, flops = 0; };
  std::map<std::string, Entry> per_shape;
  void next_pair(hipEvent_t* a, hipEvent_t* b, double fl, const std::string& what);
  void collect(int* launches, double* total_ms, double* total_flops);
  ~KernelProfiler();
};
extern thread_local KernelProfiler* g_conv_prof;

// online tile-configuration autotuner of the implicit-GEMM kernel (conv_gemm.hip)
struct ConvTuner {
  bool enabled = false;
  void* scratch = nullptr;   // device scratch for redirected outputs while timing
  size_t scratch_bytes = 0;
  int shapes_tuned = 0;
};
extern ConvTuner g_conv_tuner;

// weight repack: fp32 [N][Cin][KH][KW] (torch conv / linear with KH=KW=1) -> bf16 [Npad][KH*KW*Cpad]
// with zero padding; `geglu` interleaves value/gate rows in blocks of 32 (see conv_gemm.hip).
void launch_repack_weight(hipStream_t st, const float* w, bf16_t* out, int N, int Cin, int KH,
                          int KW, int Npad, int Cpad, int geglu, int64_t src_row_offset);

// ---------------------------------------------------------------- normalisation / softmax (norm.hip)
struct GroupNormParams {
  const bf16_t* x = nullptr;   // NHWC bf16 [B][HW][C] (optionally a channel concat of two tensors)
  const bf16_t* x1 = nullptr;
  int C0 = 0, C1 = 0, ld0 = 0, ld1 = 0;
  int B = 0, HW = 0, G = 32;
  float eps = 1e-5f;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  // FiLM (use_scale_shift_norm, improved_ddpm/unet.py:253-257): y = gn(x)*(1+scale[b][c]) + shift[b][c]
  const float* film = nullptr;  // [B][2*C]: scale | shift
  int film_ld = 0;
  int silu = 0;
  int split_out = 0;            // fp32 path only: y is the fp16 pair [B][HW][hi(C) | lo(C)] (CD_PREC_F32X3)
  int* overflow = nullptr;      // ... set to 1 by any value outside the fp16 range after scaling (host-visible word)
  bf16_t* y = nullptr;          // [B][HW][C] dense
  float* partial = nullptr;     // workspace [B][S][G][2]
  int S = 0;
  float* coef = nullptr;        // workspace [B][2][C]: per-channel multiply-add coefficients
  // statistics already produced by the conv epilogue that wrote x / x1 (ConvGemmParams::stats layout,
  // [B*HW/32][2][C]): when set, the stats pass is replaced by a small per-(image, group) fold
  const float* pre0 = nullptr;
  const float* pre1 = nullptr;
  int no_apply = 0;  // 1: stop after the coefficients (the consumer applies them itself: lin_stream.hip's proj_in variant)
};
int groupnorm_slabs(int B, int HW, int C);
void launch_groupnorm(hipStream_t st, const GroupNormParams& p);

void launch_layernorm(hipStream_t st, const bf16_t* x, int ldx, bf16_t* y, int ldy, int rows,
                      int C, const float* gamma, const float* beta, float eps);
// row softmax over fp32 scores [rows][cols] -> bf16 probabilities (VAE AttnBlock, model.py:193)
void launch_softmax_rows(hipStream_t st, const float* s, int lds, bf16_t* p, int ldp, int64_t rows,
                         int cols);

// ---------------------------------------------------------------- attention (attn.hip)
struct AttnParams {
  const bf16_t* q = nullptr;   // [B][Tq][ldq], head h at column h*D
  const bf16_t* k = nullptr;   // [B][Tk][ldk]
  // values, exactly one of:
  const bf16_t* v = nullptr;   //   token-major [B][Tk][ldv], head h at column h*D (fused q|k|v projection output)
  const bf16_t* vt = nullptr;  //   transposed: [B][H][Dv_pad][Tk_pad]  (keys contiguous)
  int ldv = 0; int64_t v_bs = 0;
  bf16_t* o = nullptr;         // [B][Tq][ldo]
  int B = 0, H = 0, Tq = 0, Tk = 0, D = 0;
  int ldq = 0, ldk = 0, ldo = 0;
  int64_t q_bs = 0, k_bs = 0, o_bs = 0;
  int vt_dpad = 0, vt_tpad = 0;
  float scale = 1.0f;            // softmax scale; ignored when q_log2 is set
  int q_log2 = 0;                // 1: q already carries scale * log2(e) (folded into the packed to_q weights)
  const float* obias = nullptr;  // [H*D] added to the output (value-projection bias: rows of P sum to 1)
  int causal = 0;                // 1: key j is visible to query i only if j <= i (CLIP text transformer)
};
void launch_attention(hipStream_t st, const AttnParams& p);
// Cross-attention control (prompt-to-prompt on the coupled loop): controlled row b takes
//   O = softmax(Q_src K_src^T) V_a + softmax(Q_own K_own^T) V_b
// with the source tensors of row src = b % B_src. V_a / V_b carry the mapper, alpha and the re-weighting
// (launch_ctrl_values); neither softmax is renormalised afterwards.
constexpr int kCtrlKeys = 96;  // keys resident in LDS per source: the context length may not exceed it
struct CtrlAttnParams {
  const bf16_t* q_own = nullptr;  // [B][Tq][ldq], head h at column h*D
  const bf16_t* q_src = nullptr;  // [B_src][Tq][ldq]
  const bf16_t* k_own = nullptr;  // [B][L][ldk]
  const bf16_t* k_src = nullptr;  // [B_src][L][ldk]
  const bf16_t* va = nullptr;     // [B][L][ldv] token-major
  const bf16_t* vb = nullptr;     // [B][L][ldv]
  bf16_t* o = nullptr;            // [B][Tq][ldo]
  int B = 0, B_src = 0, H = 0, Tq = 0, L = 0, D = 0;
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  int64_t q_bs = 0, k_bs = 0, v_bs = 0, o_bs = 0;
  float scale = 1.0f;  // softmax scale; ignored when q_log2 is set
  int q_log2 = 0;
};
void launch_cross_attention_ctrl(hipStream_t st, const CtrlAttnParams& p);
// V_a[r][i][:] = sum_j M[s][i][j] alpha[s][j] w[s][j] V[r][j][:], V_b[r][j][:] = (1 - alpha[s][j]) w[s][j] V[r][j][:] with
// s = r % B_ctrl; fp32 accumulation, one rounding. v / va / vb [rows][L][C] dense; M [B_ctrl][L][L], alpha / w [B_ctrl][L] fp32
void launch_ctrl_values(hipStream_t st, const bf16_t* v, const float* M, const float* alpha, const float* w, int rows,
                        int B_ctrl, int L, int C, bf16_t* va, bf16_t* vb);
// Per-word cross-attention maps: the score and softmax half of the control kernel, reduced in the same pass to
//   maps[r][n][q] = (1/H) * sum_hd ( sum_j sel[r % B_sel][n][j] * P_hd[q][j] ),   P = softmax over the L keys, hd ascending
// No probability is stored; fp32 from the scores on.
constexpr int kMapWords = 8;  // selector rows (words) of one launch
struct WordMapParams {
  const bf16_t* q = nullptr;   // [B][Tq][ldq], head h at column h*D
  const bf16_t* k = nullptr;   // [B][L][ldk]
  const float* sel = nullptr;  // [B_sel][N][L] weights over the key positions
  float* maps = nullptr;       // [B][N][Tq]
  int B = 0, B_sel = 0, H = 0, Tq = 0, L = 0, D = 0, N = 0;
  int ldq = 0, ldk = 0;
  int64_t q_bs = 0, k_bs = 0;
  float scale = 1.0f;  // softmax scale; ignored when q_log2 is set
  int q_log2 = 0;
};
void launch_cross_attention_maps(hipStream_t st, const WordMapParams& p);
// V [B][Tk][ldv] (head h at column h*D) -> Vt [B][H][Dpad][Tpad], zero padded
void launch_transpose_v(hipStream_t st, const bf16_t* v, int ldv, int64_t v_bs, bf16_t* vt, int B,
                        int H, int Tk, int D, int Dpad, int Tpad);

// ---------------------------------------------------------------- diagnostics (diag.hip)
// sustained 16-bit MFMA rate of this device under its power cap: bare MFMA loop on every CU for ~target_ms
void launch_mfma_sustained(hipStream_t st, int target_ms, float* tflops, float* ghz);

// ---------------------------------------------------------------- elementwise (elementwise.hip)
// fp32 NCHW [B][C][HW] -> bf16 NHWC [B][HW][Cpad] (pad channels zero), y = x*scale + shift; dup: the number of further copies
// of the B rows written behind them
void launch_nchw_to_nhwc(hipStream_t st, const float* x, bf16_t* y, int B, int C, int HW, int Cpad,
                         float scale, float shift, int dup);
// fp32/bf16 NHWC (ld) -> fp32 NCHW, y = x*scale + shift
void launch_nhwc_to_nchw(hipStream_t st, const void* x, int x_f32, int ldx, float* y, int B, int C,
                         int HW, float scale, float shift);
// sinusoidal timestep embedding -> fp32 [B][dim]; mode 0: [cos|sin], freq = exp(-ln(1e4)*k/half)
// (util.py:152-172); mode 1: [sin|cos], divisor half-1 (ddpm/diffusion.py:6-24)
void launch_timestep_embedding(hipStream_t st, const StepCoef* tab, int step, const float* t_explicit,
                               float* out, int B, int dim, int mode);
// small dense layer on fp32 vectors: y[b][n] = act_out(sum_k act_in(x[b][k])*W[n][k] + bias[n]); W bf16 or f32
void launch_vec_linear(hipStream_t st, const float* x, int ldx, const float* W, const float* bias,
                       float* y, int ldy, int B, int K, int N, int silu_in, int silu_out);
// 2x2 average pool on NHWC bf16 (improved_ddpm Downsample without conv, unet.py:132-135)
void launch_avgpool2(hipStream_t st, const bf16_t* x, bf16_t* y, int B, int H, int W, int C);
// nearest x2 upsample (materialised; only where it cannot be folded into a conv)
void launch_upsample2(hipStream_t st, const bf16_t* x, bf16_t* y, int B, int H, int W, int C);
// output of a phase-form x2 conv (ConvGemmParams::up_phase) into image order: x [B][2 a + b][H][W][C] (dense) ->
// y [B][2 y + a][2 x + b][ldy], 16-byte vectors (C and ldy multiples of 8)
void launch_up_phase_reorder(hipStream_t st, const bf16_t* x, bf16_t* y, int B, int H, int W, int C, int ldy);
// DiagonalGaussianDistribution sample (distributions.py:24-37) from moments NHWC fp32 [B][HW][2*zc]:
// z = (mean + exp(0.5*clamp(logvar,-30,20))*noise) * scale -> fp32 NCHW [B][zc][HW]
void launch_posterior_sample(hipStream_t st, const float* mom, int ld, const float* noise,
                             uint64_t seed, float* z, int B, int zc, int HW, float scale,
                             int use_mean);
// VectorQuantizer2.forward of taming-transformers (git master; not vendored by the reference, README.md:85-91) as
// VQModelInterface.decode calls it (autoencoder.py:274-282): per latent vector z (fp32 NCHW * in_mul) the nearest
// codebook row by d = (|z|^2 + |e|^2) - 2 z.e (first minimum), output z + (e - z) -> 16-bit NHWC padded to Cpad
void launch_vq_quantize(hipStream_t st, const float* z, float in_mul, const float* codebook, int n_embed, int zc,
                        int B, int HW, bf16_t* out, int Cpad);
void launch_fill_f32(hipStream_t st, float* p, float v, int64_t n);
// ViT token assembly (OpenAI CLIP VisionTransformer.forward): out[b][0] = cls + pos[0]; out[b][1+t] = patch[b][t] + pos[1+t]
void launch_vit_tokens(hipStream_t st, const bf16_t* patch, const float* cls, const float* pos, bf16_t* out, int B,
                       int T, int D);
// out[b][:] = x[b][argmax_l ids[b][l]][:]  (CLIP text pooling at the end-of-text token, the largest id)
void launch_gather_eot(hipStream_t st, const bf16_t* x, const int* ids, bf16_t* out, int B, int L, int D);
// token + position embedding lookup: out[b][l][:] = tok[ids[b][l]][:] + pos[l][:] (fp32 tables -> 16-bit rows)
void launch_embed_tokens(hipStream_t st, const int* ids, const float* tok, const float* pos, bf16_t* out, int B,
                         int L, int D, int vocab);
// ---------------------------------------------------------------- fp32 execution path (f32_path.hip)
// The same parameter structs with every activation / weight / output pointer holding fp32 data and every `ld` counted
// in floats (precision CD_PREC_F32: pixel-space DDPMs). Fixed tile shapes, no autotuner, no split-K.
void launch_conv_gemm_f32(hipStream_t st, const ConvGemmParams& p);
size_t groupnorm_f32_workspace(int B, int HW, int C);
void launch_groupnorm_f32(hipStream_t st, const GroupNormParams& p, void* workspace);
// softmax(scale * q k^T) v + obias on token-major fp32 tensors, head h at column h*D
void launch_attention_f32(hipStream_t st, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                          float* o, int ldo, int B, int H, int T, int D, float scale, const float* obias);
// split = 1: the fp16 pair form [pixel][hi(Cpad) | lo(Cpad)] of CD_PREC_F32X3 (same bytes), range guard in `overflow`
void launch_nchw_to_nhwc_f32(hipStream_t st, const float* x, float* y, int B, int C, int HW, int Cpad, float scale,
                             float shift, int split = 0, int* overflow = nullptr);
void launch_avgpool2_f32(hipStream_t st, const float* x, float* y, int B, int H, int W, int C);
// fp32 SpatialTransformer pieces (st_f32.hip): flash attention on fp32 MFMA (q, k, v token-major [B][T][ld] with the head
// at column h * D; qmul multiplies q - scale * log2 e, or 1 when the to_q rows already carry it), LayerNorm (optionally
// written as the split mode's fp16 pair), GEGLU on a materialised [rows][2 * Nout] projection in packed column order
void launch_flash_f32(hipStream_t st, const float* q, int ldq, int64_t q_bs, const float* k, int ldk, int64_t k_bs,
                      const float* v, int ldv, int64_t v_bs, float* o, int ldo, int64_t o_bs, int B, int H, int Tq, int Tk,
                      int D, float qmul, int split, int* overflow, const float* obias = nullptr);
void launch_layernorm_f32(hipStream_t st, const float* x, int ldx, float* y, int64_t rows, int C, const float* gamma,
                          const float* beta, float eps, int split, int* overflow);
void launch_geglu_f32(hipStream_t st, const float* h, float* y, int64_t rows, int Nout, int split, int* overflow);
void launch_split_rows_f32(hipStream_t st, const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, bf16_t* y,
                           int64_t rows, int* overflow);
void launch_upsample2_f32(hipStream_t st, const float* x, float* y, int B, int H, int W, int C);
// Split-fp16 mode of the fp32 path (precision CD_PREC_F32X3): a GroupNorm-ed activation x is kept as the fp16 pair
// T = [hi | lo] per pixel, hi = fp16(s_a x), lo = fp16(s_a x - hi), and a weight as [wh | wh | wl] per filter tap
// (scaled by s_w), so that one 16-bit implicit GEMM over the channel list [hi | lo | hi] with alpha = 1 / (s_a s_w)
// yields x.w to 2^-22 (the lo.wl term is dropped). Exact powers of two; fp16 builds only.
constexpr float kX3ActScale = 16.f;    // |x| < 4095 representable, full 22 bits down to |x| = 2^-6, 2^-28 absolute below
constexpr float kX3WgtScale = 256.f;   // |w| < 255, full 22 bits down to |w| = 2^-10
// fp32 packed weights [Npad][taps][Cpad] -> 16-bit [Npad][taps][3 * Cpad]
// `overflow` (may be null): a host-visible word the kernels set to 1 when a scaled value leaves the fp16 range - the
// engine turns it into an error at its next synchronisation point instead of returning saturated results.
void launch_pack_w3(hipStream_t st, const float* w, bf16_t* w3, int Npad, int taps, int Cpad, int* overflow);
// 2 x 2 average pool of a split activation [B][H][W][2C] -> [B][H/2][W/2][2C]
void launch_avgpool2_split(hipStream_t st, const bf16_t* x, bf16_t* y, int B, int H, int W, int C, int* overflow);

void launch_copy_strided_bf16(hipStream_t st, const bf16_t* src, int lds, bf16_t* dst, int ldd,
                              int64_t rows, int cols);

// ---------------------------------------------------------------- FID Inception-v3 (inception.hip)
// 3 x 3 pool over 16-bit NHWC: x [B][H][W] pixels of stride ldx -> y [B][Ho][Wo] pixels of stride ldy, Ho = (H + 2 pad - 3) /
// stride + 1. max: the maximum of the in-image taps, else their mean (count_include_pad = False). C, ldx, ldy multiples of 8.
void launch_pool3x3(hipStream_t st, const bf16_t* x, int ldx, int B, int H, int W, int C, bool max, int stride, int pad,
                    bf16_t* y, int ldy);
// global average pool: x [B][HW] pixels of stride ldx, C channels (C, ldx multiples of 8) -> y fp32 [B][C]
void launch_global_avg(hipStream_t st, const bf16_t* x, int ldx, int B, int HW, int C, float* y);
// BatchNorm (eps 1e-3, torchvision BasicConv2d) folded into a conv: raw fp32 [N][Cin][KH][KW] -> rows n < N of the packed
// 16-bit [Npad][KH][KW][Cpad], w' = w * gamma / sqrt(var + eps) (channels Cin.. zero), bias[n] = beta - mean * gamma / sqrt(var + eps)
void launch_fold_bn(hipStream_t st, const float* raw, const float* gamma, const float* beta, const float* mean, const float* var,
                    int N, int Cin, int KH, int KW, int Cpad, bf16_t* w, float* bias);
// the implicit-GEMM launch of one BasicConv2d (conv + folded BatchNorm + ReLU): x [B][H][W] pixels of stride ldx, Cpad channels
// read; wgt / bias as launch_fold_bn leaves them; N rounded up to 32 columns (the extra weight rows and bias entries are zero, so
// the GEMM writes the zero padding channels the next layer reads); out [B * Hout * Wout] rows of stride out_ld
ConvGemmParams basic_conv_params(const bf16_t* x, int ldx, int B, int H, int W, int Cpad, const bf16_t* wgt, const float* bias,
                                 int N, int KH, int KW, int stride, int pad_t, int pad_l, void* out, int out_ld,
                                 const bf16_t* zeros);

// ---------------------------------------------------------------- LPIPS (lpips.hip)
// the package's scaling layer and the layout change in one pass: x fp32 NCHW [B][3][HW] -> y 16-bit NHWC [B][HW][32],
// channel c < 3 = (x - shift[c]) / scale[c], channels 3..31 zero
void launch_lpips_input(hipStream_t st, const float* x, bf16_t* y, int B, int HW);
// 2 x 2 stride-2 max pool over 16-bit NHWC (floor of odd sizes): x [B][H][W] pixels of stride ldx -> y [B][H / 2][W / 2] pixels
// of stride ldy. C, ldx, ldy multiples of 8.
void launch_pool2x2(hipStream_t st, const bf16_t* x, int ldx, int B, int H, int W, int C, bf16_t* y, int ldy);
// one LPIPS tap: f0, f1 16-bit [B][HW] pixels of stride ld, C channels (C % 8 == 0, C <= 512, ld % 8 == 0), w fp32 [C]:
//   d[b] = mean over pixels of sum_c w[c] (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2
// part: fp32 scratch [B][lpips_layer_chunks(HW, C)]. per_layer (or null) [B][5] gets d at column `layer`; out[b] = d[b], or
// out[b] += d[b] when `accumulate`. No atomics: the same bits for an image whatever the batch around it.
int lpips_layer_chunks(int HW, int C);
void launch_lpips_layer(hipStream_t st, const bf16_t* f0, const bf16_t* f1, int ld, int B, int HW, int C, const float* w,
                        float* part, float* per_layer, int layer, bool accumulate, float* out);

}  // namespace cd

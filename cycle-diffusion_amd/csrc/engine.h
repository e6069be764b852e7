// Engine core: device arena, parameter store keyed by the reference's state_dict names, and the
// network executors (static launch schedules over the kernels in kernels.h).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "../../include/cyclediff.h"

namespace cd {

// ------------------------------------------------------------------ device memory
// Stack-discipline bump allocator over one slab (sized for 288 GB parts: activations of a whole
// forward pass stay resident; temporaries of a block are released at block exit so the hot
// working set keeps re-using the same lines of the 256 MiB Infinity Cache).
class Arena {
 public:
  ~Arena();
  void init(size_t bytes);
  void* alloc(size_t bytes);
  size_t mark() const { return off_; }
  void release(size_t m) { off_ = m; }
  void reset() { off_ = 0; }
  size_t capacity() const { return cap_; }
  size_t high_water() const { return high_; }
 private:
  char* base_ = nullptr;
  size_t cap_ = 0, off_ = 0, high_ = 0;
};

struct Act {  // NHWC activation view: 16-bit elements, or fp32 when f32 is set (precision CD_PREC_F32)
  bf16_t* p = nullptr;
  int B = 0, H = 0, W = 0, C = 0;
  int ld = 0;  // pixel stride (elements)
  bool f32 = false;
  // fp32 path in the split-fp16 mode (CD_PREC_F32X3): p holds the fp16 pair [hi(C) | lo(C)] per pixel, ld = 2 * C
  // (kernels.h kX3ActScale). Only GroupNorm outputs (and their 2x2 average pools) take this form; convs consume it
  bool split = false;
  float* pf() const { return (float*)p; }
  // GroupNorm statistics of this tensor, written by the conv epilogue that produced it
  // ([B*H*W/32][2][C] fp32, ConvGemmParams::stats); stats_buf = storage, stats = valid content
  float* stats = nullptr;
  float* stats_buf = nullptr;
  int64_t rows() const { return (int64_t)B * H * W; }
};

// ------------------------------------------------------------------ parameters
struct ConvW {  // packed conv / linear weight: 16-bit (or fp32 when f32) [Npad][KH*KW*Cpad], fp32 bias[N]
  bf16_t* w = nullptr;
  bf16_t* wfrag = nullptr;  // the same rows in MFMA-fragment-major order for lin_stream.hip (1x1, 320 input channels)
  bf16_t* w3 = nullptr;     // CD_PREC_F32X3: fp16 [Npad][KH*KW][wh | wh | wl] (3 * Cpad per tap), from the fp32 rows in w
  // 3 x 3 weights of a nearest-x2 conv, 16-bit path: the four 2 x 2 phase matrices [2 a + b][Npad][2 * 2 * Cpad] derived from w
  // (ParamStore::add_up_phase / refresh_up_phase; ConvGemmParams::up_phase), or null
  bf16_t* wphase = nullptr;
  int wphase_version = -1;  // ParamStore::version the phase matrices were built at
  bool f32 = false;
  float* b = nullptr;
  int N = 0, Cin = 0, Cpad = 0, KH = 1, KW = 1, Npad = 0;
  bool geglu = false;
  int Ktot() const { return KH * KW * Cpad; }
};

struct PackTarget {
  enum Kind { MATRIX_BF16, VECTOR_F32, MATRIX_F32 } kind;
  // MATRIX_BF16: rows [dst_row0, dst_row0+rows) of dst ConvW come from source rows
  //   src_base + (j/grp)*grp_stride + j%grp, j in [0, rows)
  ConvW* conv = nullptr;
  int dst_row0 = 0, rows = 0, src_base = 0, grp = 0, grp_stride = 0;
  // VECTOR_F32 / MATRIX_F32: dst[dst_off + j(*K)] with the same row mapping; geglu interleave
  float* fdst = nullptr;
  int dst_off = 0, K = 1;
  bool geglu = false;
  int geglu_N = 0;
  float scale = 1.f;  // rows are multiplied by this before the one rounding to the packed format
};

struct ParamDecl {
  std::string name;
  std::vector<int64_t> shape;  // reference (torch) shape
  std::vector<PackTarget> targets;
  bool loaded = false;
  bool transposed = false;  // reference tensor is [K][N] (used as x @ W); rows are transposed on load
};

class ParamStore {
 public:
  ~ParamStore();
  bool f32 = false;  // matrices are packed as fp32 (set by the network before it declares anything)
  bool x3 = false;   // ... and additionally as three-term fp16 splits (CD_PREC_F32X3)
  int* overflow = nullptr;  // host-visible word set when a split weight leaves the fp16 range (engine-owned)
  int version = 0;   // bumped by every load(): derived weights (LayerNorm folds) are rebuilt when it moves
  // allocate packed storage
  ConvW* new_conv(int N, int Cin, int KH, int KW, bool bias, bool geglu = false);
  float* new_vec(int n, float init = 0.f);
  // storage for the phase matrices of a 3 x 3 x2-upsample conv (16-bit path only; a no-op elsewhere), and their rebuild
  // from the loaded weights when the store has changed since the last one (stream-ordered, microseconds)
  void add_up_phase(ConvW* c);
  void refresh_up_phase(hipStream_t st, ConvW* c);
  // declare reference tensors and where their rows go
  ParamDecl& declare(const std::string& name, std::vector<int64_t> shape);
  // whole tensor -> whole ConvW; ref_ndim = rank of the reference tensor (2 Linear, 3 Conv1d, 4 Conv2d; 0 = auto)
  // scale: folded into the rows before they are rounded (attention: softmax scale * log2(e) into to_q)
  void conv_weight(const std::string& name, ConvW* c, int ref_ndim = 0, float scale = 1.f);
  // reference tensor of shape [Cin][N] applied as `x @ W` (OpenAI CLIP `proj` / `text_projection`)
  void conv_weight_t(const std::string& name, ConvW* c);
  void conv_bias(const std::string& name, ConvW* c);
  void conv_rows(const std::string& name, std::vector<int64_t> shape, ConvW* c, int dst_row0, int rows,
                 int src_base, int grp, int grp_stride, float scale = 1.f);
  void bias_rows(const std::string& name, int64_t n_total, float* dst, int dst_off, int rows, int src_base,
                 int grp, int grp_stride);
  void vec(const std::string& name, float* dst, int n);
  void mat_f32(const std::string& name, float* dst, int N, int K, int dst_row0 = 0);

  void load(hipStream_t st, const std::string& name, const float* host, int ndim, const int64_t* shape);
  int missing(std::string* first = nullptr) const;
  const std::vector<std::unique_ptr<ParamDecl>>& decls() const { return decls_; }
  size_t device_bytes() const { return dev_bytes_; }
 private:
  std::vector<std::unique_ptr<ParamDecl>> decls_;
  std::map<std::string, ParamDecl*> by_name_;
  std::vector<std::unique_ptr<ConvW>> convs_;
  std::vector<void*> allocs_;
  float* staging_ = nullptr;
  size_t staging_bytes_ = 0;
  size_t dev_bytes_ = 0;
  void* dmalloc(size_t bytes);
};

// ------------------------------------------------------------------ execution context
struct Ctx {
  hipStream_t st = nullptr;
  Arena* arena = nullptr;
  const bf16_t* zeros = nullptr;
  float* gn_partial = nullptr;  // [B][S][G][2] scratch, sized for the largest GroupNorm
  size_t gn_partial_floats = 0;
  bool f32 = false;             // the running network executes in fp32 (Net::f32)
  bool x3 = false;              // ... with its GroupNorm-fed convolutions as three-term fp16 GEMMs (Net::x3)
  int* overflow = nullptr;      // host-visible word the split kernels set on a value outside the fp16 range
};
// A network's precision flags on the context for the length of one forward (or of its context projections); the previous
// ones are back on exit, also when a CD_CHECK throws
class PrecisionScope {
 public:
  PrecisionScope(Ctx& c, bool f32, bool x3) : c_(c), f32_(c.f32), x3_(c.x3) { c.f32 = f32; c.x3 = x3; }
  ~PrecisionScope() { c_.f32 = f32_; c_.x3 = x3_; }
  PrecisionScope(const PrecisionScope&) = delete;
  PrecisionScope& operator=(const PrecisionScope&) = delete;
 private:
  Ctx& c_;
  const bool f32_, x3_;
};

// shared building blocks -------------------------------------------------------------------
struct ConvOpts {
  int stride = 1;
  int pad = 1;          // symmetric top/left padding (bottom/right implied by the output size)
  bool asym = false;    // VAE/Ho Downsample: F.pad(x,(0,1,0,1)) + stride-2 conv (model.py:72-76)
  bool up = false;      // nearest x2 before the conv
  const float* rowvec = nullptr; int rowvec_ld = 0; int rows_per_vec = 1;
  const Act* resid = nullptr;
  int act = ACT_NONE;
  float alpha = 1.f;
  bool out_f32 = false;
  void* out = nullptr;  // optional preallocated output
  int out_ld = 0;
  // LayerNorm the input rows inside the kernel (statistics only; the weights carry gain and bias): the streaming
  // K = 320 linear kernel only - the caller checks conv_ln_fold_available() first
  bool ln_fold = false;
  float ln_eps = 1e-5f;
  bool raw_geglu = false;      // fp32 path: a GEGLU projection leaves its [value | gate] columns as they are (k_geglu_f32 follows)
  bool want_stats = false;     // output feeds a GroupNorm: emit its statistics from the epilogue
  float* out_stats = nullptr;  // storage for them when `out` is preallocated
  int tile = 0;
};
// fp32 path, transformer blocks (st_f32.hip): q [B][Tq][ldq], k / v [B][Tk][ld] fp32 with per-image strides
Act attention_flash_f32_fwd(Ctx& c, const float* q, int ldq, const float* k, int ldk, int64_t k_bs, const float* v, int ldv,
                            int64_t v_bs, int B, int H, int Tq, int Tk, int D, float scale, int Himg, int Wimg, bool q_log2);
Act geglu_f32_fwd(Ctx& c, const Act& h);
Act split_rows_f32_fwd(Ctx& c, const Act& x, const Act* x2 = nullptr);  // split mode: fp32 rows (or a channel concat) as fp16 pairs (range-guarded)  // [rows][2 * Nout] packed [32 value | 32 gate] blocks -> [rows][Nout]
Act alloc_act(Ctx& c, int B, int H, int W, int C, bool with_stats = false);
// y = conv(x [| x2]) with the fused epilogue; returns the output view (bf16 unless out_f32)
Act conv_fwd(Ctx& c, const ConvW& w, const Act& x, const Act* x2, const ConvOpts& o);
// whether conv_fwd runs this nearest-x2 3 x 3 conv as four 2 x 2 phase convs on the stored grid (CYCLEDIFF_UP_PHASE=0: never)
bool conv_up_phase_taken(const Ctx& c, const ConvW& w, const Act& x, const Act* x2, const ConvOpts& o);
// whether a LayerNorm-folded call of this layer on `rows` tokens would run (streaming kernel applicable and the shape
// large enough for it to be the fastest choice: the 64 x 64 level from 16 images up)
bool conv_ln_fold_available(const Ctx& c, const ConvW& w, int64_t rows);

struct GNW { float* g = nullptr; float* b = nullptr; int C = 0; float eps = 1e-5f; };
Act groupnorm_fwd(Ctx& c, const GNW& w, const Act& x, const Act* x2, bool silu, const float* film = nullptr,
                  int film_ld = 0);
struct LNW { float* g = nullptr; float* b = nullptr; int C = 0; };
Act layernorm_fwd(Ctx& c, const LNW& w, const Act& x);
// 16-bit path, single source, no SiLU / FiLM: the statistics passes of groupnorm_fwd without the apply pass. Returns the
// per-image multiply-add coefficients [B][2][C] (al | be), valid until the next GroupNorm of this engine is launched
const float* groupnorm_coef_fwd(Ctx& c, const GNW& w, const Act& x);
// declarations under the reference's state_dict prefix `pfx`: the gain and bias of a norm, the weight (and bias) of a k x k
// conv or linear layer. ref_ndim: rank of the reference weight tensor (2 = nn.Linear, 3 = Conv1d, 4 = Conv2d)
GNW make_gn(ParamStore& ps, const std::string& pfx, int C, float eps);
LNW make_ln(ParamStore& ps, const std::string& pfx, int C);
ConvW* make_conv(ParamStore& ps, const std::string& pfx, int N, int Cin, int k, bool bias = true, bool geglu = false,
                 int ref_ndim = 4, float wscale = 1.f);
// the network's input rows [B][H][W][C] as the caller laid them out: 16-bit, fp32, or - a split-mode network - fp16 pairs
Act net_input_act(const void* p, int B, int H, int W, int C, bool f32, bool x3);

// Residual block of the four conv nets: GroupNorm -> SiLU -> conv3x3 (+ the block's row of the time embedding) -> GroupNorm
// (FiLM: scaled and shifted by that row instead) -> SiLU -> conv3x3, plus the input, through a 1 x 1 projection when the
// channels change; up / down: resblock_updown (improved_ddpm/unet.py:104-135). The networks declare the weights under
// their own state_dict names and assign emb_off.
struct ResW {
  int cin = 0, cout = 0;
  bool up = false, down = false, film = false;
  GNW gn1, gn2;
  ConvW *conv1 = nullptr, *conv2 = nullptr, *skip = nullptr;
  int emb_off = -1;  // offset into the fused time-embedding projection; -1 = no embedding row (the first stage)
};
// x2: second source of a channel concat, or null; proj [1 or B][proj_ld]: time_emb_fwd's rows
Act res_fwd(Ctx& c, const ResW& r, const Act& x, const Act* x2, const float* proj, int proj_ld, bool t_shared);

// Attention block on image tokens: GroupNorm -> q | k and v projections -> softmax(D^-1/2 q k^T) v + vbias per head of
// width D = C / heads -> proj_out, plus the input
struct AttnW {
  int C = 0, heads = 1;
  GNW norm;
  ConvW *qk = nullptr, *v = nullptr, *proj = nullptr;  // [Wq; Wk] with bias, Wv without (vbias is added to the output)
  float* vbias = nullptr;
};
Act attn_block_fwd(Ctx& c, const AttnW& a, const Act& x);

// Entry of a SpatialTransformer block of the 320-channel level with d_head = 40 (16-bit path): GroupNorm -> proj_in ->
// LayerNorm1 -> to_q | to_k -> V^T. On whole images of a multiple of 256 tokens and enough rows for the streaming kernel
// (st_entry_available) the three norm / transpose launches run inside the two k_lin_stream launches:
enum {
  ST_ENTRY_QKV = 1,  // one q | k | v launch whose last 320 columns leave as V^T (no V^T GEMM); same bits
  ST_ENTRY_LN1 = 2,  // ... with LayerNorm1 in its registers and its gain / bias in its weights (needs ST_ENTRY_QKV)
  ST_ENTRY_GN = 4,   // GroupNorm's multiply-add applied in proj_in's registers (no apply pass); same bits
};
int st_entry_stages();  // CYCLEDIFF_ST_ENTRY (a bit per stage, default all), read once: A/B runs
// where the launches are valid and sensible at all (whole images per strip, >= 32 768 rows); the norm1 fold is gated by
// conv_ln_fold_available on top
bool st_entry_available(const Ctx& c, int64_t rows, int hw);
// where the U-Net takes them: the row counts at which the shipped tile table already runs proj_in and q | k on the streaming
// kernel (tune_gfx950.txt: tile 30 for N = 320 and N = 640 from 61 440 rows of 64 x 64 tokens). Smaller forwards - the coupled
// single batch's 49 152 rows among them - keep their tiles and their separate norm launches.
constexpr int64_t kStEntryNetMinRows = 61440;
struct StEntryW {
  GNW norm; LNW ln1;
  const ConvW *proj_in = nullptr, *qk1 = nullptr, *v1 = nullptr;
  // derived, not declared as parameters (st_entry_refresh): [Wq*; Wk; Wv] fragment-major with a zero bias (or vbias for
  // the value rows), and the same with LayerNorm1 folded in (W diag(gamma) rounded once, bias W beta)
  ConvW *qkv = nullptr, *qkv_ln = nullptr;
  const float* vbias = nullptr;  // tests only: to_v has no bias in the reference
};
void st_entry_alloc(ParamStore& ps, StEntryW& w);
void st_entry_refresh(hipStream_t st, StEntryW& w);
struct StEntryOut { Act h, qk; bf16_t* vt = nullptr; int Tpad = 0; int stages = 0; };  // stages: the bits that ran
// V^T[b] = Wv . X[b]^T on the implicit-GEMM family: weights as the A operand, tokens as the B operand -> [B][C][Tpad]
void vt_gemm_fwd(Ctx& c, const ConvW& wv, const bf16_t* x, int ldx, int B, int T, int Tpad, bf16_t* vt);
// attn_block_fwd between its q | k projection and proj_out (16-bit path): qk [B*T][2C] and the normalised rows n [B*T][C] ->
// o = softmax(D^-1/2 q k^T) (Wv n) + vbias per head, D = C / heads. o.p == nullptr: allocated from the arena, as vt [B][C][Tpad]
// is. branch: 0 = the flash kernel (D <= 160), 1 = scores materialised once per image (the wide single head of the first stage)
struct AtCoreOut { Act o; bf16_t* vt = nullptr; int Tpad = 0; int branch = 0; };
AtCoreOut at_core(Ctx& c, const ConvW& wv, const float* vbias, const Act& qk, const Act& n, int C, int heads, Act o = Act());
// h = proj_in(GroupNorm(x)) [B*T][C]; then qk = [q (log2 units) | k] of LayerNorm1(h) [B*T][2C], vt [B][C][Tpad]
// (arena-allocated: the caller brackets the second call with the mark its attention releases); st_entry_fwd = both
Act st_entry_proj_in(Ctx& c, const StEntryW& w, const Act& x, int stages);
StEntryOut st_entry_qkv(Ctx& c, const StEntryW& w, const Act& h, int stages);
StEntryOut st_entry_fwd(Ctx& c, const StEntryW& w, const Act& x, int stages);

// 2x2 average pool / nearest x2 upsample of a dense activation (resblock_updown, improved_ddpm/unet.py:104-135)
Act avgpool2_fwd(Ctx& c, const Act& x);
Act upsample2_fwd(Ctx& c, const Act& x);
// fp32 path: softmax(scale q k^T) v + obias with q | k in one token-major tensor and v in another
Act attention_f32_fwd(Ctx& c, const Act& qk, const Act& v, int H, int D, float scale, const float* obias);

// multi-head attention on token-major activations: q [B][Tq][ldq], k [B][Tk][ldk], v [B][Tk][ldv] (head h at column
// h*D of each). q_log2: q already carries scale * log2(e) (folded into its projection weights); `scale` is then unused.
// rows >= 0: the output holds all B samples and only the first `rows` are computed (the caller's own launch writes the rest)
Act attention_fwd(Ctx& c, const bf16_t* q, int ldq, const bf16_t* k, int ldk, const bf16_t* v, int ldv, int B,
                  int H, int Tq, int Tk, int D, float scale, int Himg, int Wimg, bool q_log2 = false, int rows = -1);
// the same with V pre-transposed: vt [B][H*D][Tpad] (keys contiguous, zero padded to Tpad % 64 == 0). obias [H*D] is added to
// the output (a value bias); o.p != nullptr: the caller's output rows instead of an arena allocation
Act attention_vt_fwd(Ctx& c, const bf16_t* q, int ldq, const bf16_t* k, int ldk, const bf16_t* vt, int B,
                     int H, int Tq, int Tk, int Tpad, int D, float scale, int Himg, int Wimg, bool q_log2 = false,
                     const float* obias = nullptr, Act o = Act());

// ------------------------------------------------------------------ networks
class Net {
 public:
  virtual ~Net() {}
  ParamStore params;
  cd_net_desc desc;
  bool f32 = false;  // desc.precision is CD_PREC_F32 or CD_PREC_F32X3
  bool x3 = false;   // desc.precision == CD_PREC_F32X3
  // the flags above and those of the parameter store, ahead of the first declaration
  void set_precision(const cd_net_desc& d) {
    f32 = d.precision == CD_PREC_F32 || d.precision == CD_PREC_F32X3;
    x3 = d.precision == CD_PREC_F32X3;
    params.f32 = f32; params.x3 = x3;
  }
  virtual int kind() const = 0;
};

struct TimeEmb {  // shared by all U-Nets: sinusoid -> MLP -> per-ResBlock projections in one launch
  int mode = 0, dim = 0, hidden = 0;
  float *w0 = nullptr, *b0 = nullptr, *w1 = nullptr, *b1 = nullptr;  // fp32 [hidden][dim], [hidden][hidden]
  float* proj_w = nullptr; float* proj_b = nullptr;                   // fused emb_layers: [proj_total][hidden]
  int proj_total = 0;
};

// Cross-attention control of one forward (UNet::build_attn_control fills it once per call): rows
// [row0, row0 + rows) of the batch - always its tail - run k_cross_attention_ctrl in every text cross-attention, with the
// to_q output and the cached keys of row src_b0 + (r - row0) % B_src as the source; every other row runs k_attention.
struct AttnCtrl {
  std::vector<const bf16_t*> va, vb;  // per transformer block, [rows][L][C] (stored like the cached context values)
  int row0 = 0, rows = 0;
  int src_b0 = 0, B_src = 0;
};

// Per-word attention maps of one forward (cd_word_maps): every text cross-attention whose token grid side lies
// in the window also runs k_cross_attention_maps on its own q and cached keys and adds the result into the per-row sums `acc`.
// The attention output itself is the launch it always was. Rows are (draw i, sample b) = i * B + b.
struct WordMapCollect {
  const float* sel = nullptr;  // [B_sel][N][L] device
  int N = 0, B_sel = 0;
  int min_side = 0, max_side = 0;  // 0, 0 = every block
  float* acc = nullptr;            // [rows][N][h][w] sums over the included layers, in the forward's order
  int B = 0, n_chunk = 0;          // rows = n_chunk * B: sample b of draw i uses selector entry b % B_sel
  mutable int layers = 0;          // blocks included so far in this forward
  // The ranged form (cd_local_blend): instead of all rows of the forward, the map kernel runs once
  // per range on rows [row0, row0 + rows) with N = 1, row r of the range using selector entry r % B_sel, and the range's own
  // sums acc [rows][side][side] stay on the token grid. The sums run on across the forwards of a call: they start from 0 at
  // the first included block of the first forward (`seen` counts the blocks of all forwards). The batch may have repeated
  // rows and run cross-attention control: at attn2 every row exists, and the map kernel reads q and the cached keys only.
  struct Range {
    int row0 = 0, rows = 0;
    const float* sel = nullptr;  // [B_sel][L]
    int B_sel = 0;
    float* acc = nullptr;
  };
  std::vector<Range> ranges;
  mutable int seen = 0;
  bool ranged() const { return !ranges.empty(); }
  bool takes(int side) const { return (min_side == 0 && max_side == 0) || (side >= min_side && side <= max_side); }
};

struct UNetIO {
  const bf16_t* xin = nullptr;   // NHWC bf16 [B][H][W][Cpad_in]
  int B = 0;
  // timestep source: either a schedule table row or explicit floats
  const StepCoef* tab = nullptr; int step = 0;
  const float* t_explicit = nullptr;  // [B] device, or null
  bool t_shared = true;               // all samples share one timestep -> embed once
  // classifier-free-guidance batch [uncond B/2 | cond B/2] built from ONE x_t (ddim.py:553-559 th.cat([x] * 2)): rows
  // B/2 .. B-1 of xin repeat rows 0 .. B/2-1 and only the cross-attention context differs, so everything ahead of the
  // first cross-attention may be computed once for B/2 rows and duplicated
  bool cfg_dup = false;
  // generalisation for the coupled encode / decode loop (cd_cycle_translate): the batch is [rows 0 .. B - dup_tail - 1 unique |
  // dup_tail rows that repeat the dup_tail rows just ahead of them], e.g. [encoder rows | decoder uncond | decoder cond]
  // with dup_tail = the decoder's sample count. cfg_dup is the case dup_tail = B / 2. 0 = no repeated rows.
  int dup_tail = 0;
  const AttnCtrl* ctrl = nullptr;     // cross-attention control of this forward, or null (16-bit path only)
  const WordMapCollect* maps = nullptr;  // per-word attention maps collected beside this forward, or null (16-bit path only)
  float* out = nullptr;               // fp32 [B*H*W][out_ld]
  int out_ld = 0;
};
// sinusoid -> Linear -> SiLU -> Linear, then every ResBlock's SiLU -> Linear in one launch: the fused projection rows
// [1 or io.B][te.proj_total] fp32 (one row when the samples share the timestep), from the arena
float* time_emb_fwd(Ctx& c, const TimeEmb& te, const UNetIO& io);

class UNet : public Net {
 public:
  virtual void forward(Ctx& c, const UNetIO& io) = 0;
  // cross-attention K / V^T of the context are step-invariant: computed once per call
  virtual void set_context(Ctx& c, const bf16_t* ctx, int B, int L) { (void)c; (void)ctx; (void)B; (void)L; }
  // after set_context: V_a / V_b of every transformer block for rows [ctrl.row0, ctrl.row0 + ctrl.rows) of that context, from
  // the device tensors mapper [B_ctrl][L][L], alpha / weight [B_ctrl][L] (row r uses entry (r - row0) % B_ctrl); fills
  // ctrl.va / ctrl.vb, allocated from the arena (they live as long as the caller's arena scope).
  virtual void build_attn_control(Ctx&, const float*, const float*, const float*, int, AttnCtrl&) {
    CD_CHECK(false, "cross-attention control: the network has no text cross-attention");
  }
  // text cross-attention blocks whose token grid side lies in [min_side, max_side] (0, 0 = all); 0 without a text context
  virtual int count_text_blocks(int, int) const { return 0; }
  int in_cpad = 32;
  int out_channels = 0;
  int image_size = 0;
  virtual size_t workspace_hint(int B) const = 0;
};

std::unique_ptr<UNet> make_unet_openai(const cd_net_desc& d);
std::unique_ptr<UNet> make_unet_ho(const cd_net_desc& d);

class VAE : public Net {
 public:
  int kind() const override { return CD_NET_VAE_KL; }
  // img H x W pixels, z h x w latent cells; either extent a multiple of `factor` / any (the convolutions are fully
  // convolutional and the mid attention runs over the h * w tokens it is given)
  virtual void encode_moments(Ctx& c, const bf16_t* img_nhwc, int B, int H, int W, float* moments) = 0;  // fp32 [B*h*w][2*zc]
  virtual void decode(Ctx& c, const bf16_t* z_nhwc, int B, int h, int w, float* img) = 0;                // fp32 [B*H*W][3]
  int z_channels = 4, factor = 8;
  int moments_channels = 8;          // channels of encode_moments' output: 2 * embed_dim (KL) or embed_dim (VQ)
  const float* codebook = nullptr;   // VQ first stage: [n_embed][embed_dim] fp32, else null
  int n_embed = 0;
};
std::unique_ptr<VAE> make_vae_kl(const cd_net_desc& d);

class TextEncoder : public Net {  // token ids -> conditioning sequence
 public:
  virtual void encode(Ctx& c, const int* ids_dev, int B, int L, float* out) = 0;  // fp32 [B][L][width]
  // OpenAI-CLIP towers (DirectionalCLIP ranker): pooled + projected features fp32 [B][embed]
  virtual void text_features(Ctx&, const int*, int, int, float*) { CD_CHECK(false, "net has no pooled text features"); }
  virtual void image_features(Ctx&, const float*, int, float*) { CD_CHECK(false, "net has no image tower"); }
  virtual int width() const = 0;
  virtual int max_positions() const = 0;
};
std::unique_ptr<TextEncoder> make_clip_text(const cd_net_desc& d);

// the FID Inception-v3 (inception.hip): pool3 features [B][2048] fp32, or the fp32 NCHW output of block list entry
// stop_block >= 0 (include/cyclediff.h cd_inception_features)
std::unique_ptr<Net> make_inception_fid(const cd_net_desc& d);
void inception_fid_features(Net* n, Ctx& c, const float* img, int B, int stop_block, float* out);

// LPIPS v0.1 on the AlexNet / VGG16 features (lpips.hip): img0 / img1 fp32 NCHW [B][3][H][W] in [-1, 1] -> out [B] (and
// per_layer [B][5] when not null); lpips_tap: un-normalised ReLU output of tap 0..4 as fp32 NCHW
std::unique_ptr<Net> make_lpips(const cd_net_desc& d);
void lpips_distance(Net* n, Ctx& c, const float* img0, const float* img1, int B, int H, int W, float* per_layer, float* out);
void lpips_tap(Net* n, Ctx& c, const float* img, int B, int H, int W, int tap, float* out);

}  // namespace cd

// Executors for the pytorch_diffusion-style blocks shared by
//   * the KL-f8 autoencoder: Encoder / Decoder / AutoencoderKL.encode|decode
//     (ldm/modules/diffusionmodules/model.py:368-568, ldm/models/autoencoder.py:324-333)
//   * the Ho et al. DDPM U-Net (model/lib/ddpm_ddim/models/ddpm/diffusion.py:192-337)
// ResnetBlock: GN(eps 1e-6) -> swish -> conv3x3 (+ temb_proj(swish(temb))) -> GN -> swish -> conv3x3,
// 1x1 nin_shortcut when channels change; AttnBlock: single head over H*W tokens with d = C.
#include <algorithm>

#include "engine.h"

namespace cd {

namespace {

constexpr float kGnEps = 1e-6f;  // Normalize(): GroupNorm(32, C, eps=1e-6) (model.py:39, diffusion.py:33)

ResW mk_res(ParamStore& ps, const std::string& pfx, int cin, int cout) {
  ResW r; r.cin = cin; r.cout = cout;
  r.gn1 = make_gn(ps, pfx + ".norm1", cin, kGnEps);
  r.conv1 = make_conv(ps, pfx + ".conv1", cout, cin, 3);
  r.gn2 = make_gn(ps, pfx + ".norm2", cout, kGnEps);
  r.conv2 = make_conv(ps, pfx + ".conv2", cout, cout, 3);
  if (cin != cout) r.skip = make_conv(ps, pfx + ".nin_shortcut", cout, cin, 1);
  return r;
}
AttnW mk_at(ParamStore& ps, const std::string& pfx, int C) {
  AttnW a; a.C = C;
  a.norm = make_gn(ps, pfx + ".norm", C, kGnEps);
  a.qk = ps.new_conv(2 * C, C, 1, 1, true);
  ps.conv_rows(pfx + ".q.weight", {C, C, 1, 1}, a.qk, 0, C, 0, C, 0);
  ps.conv_rows(pfx + ".k.weight", {C, C, 1, 1}, a.qk, C, C, 0, C, 0);
  ps.bias_rows(pfx + ".q.bias", C, a.qk->b, 0, C, 0, C, 0);
  ps.bias_rows(pfx + ".k.bias", C, a.qk->b, C, C, 0, C, 0);
  a.v = ps.new_conv(C, C, 1, 1, false);
  ps.conv_weight(pfx + ".v.weight", a.v, 4);
  a.vbias = ps.new_vec(C);
  ps.vec(pfx + ".v.bias", a.vbias, C);
  a.proj = make_conv(ps, pfx + ".proj_out", C, C, 1);
  return a;
}

// ================================================================== KL autoencoder
class VAEKL : public VAE {
 public:
  explicit VAEKL(const cd_net_desc& d);
  void encode_moments(Ctx& c, const bf16_t* img, int B, int H, int W, float* moments) override;
  void decode(Ctx& c, const bf16_t* z, int B, int h, int w, float* img) override;
 private:
  int ch_, nres_, nlev_;
  std::vector<int> mult_;
  // encoder
  ConvW* e_in_ = nullptr; std::vector<std::vector<ResW>> e_blk_; std::vector<ConvW*> e_down_;
  ResW e_m1_, e_m2_; AttnW e_at_; GNW e_no_; ConvW* e_out_ = nullptr; ConvW* quant_ = nullptr;
  // decoder
  ConvW* pq_ = nullptr; ConvW* d_in_ = nullptr; ResW d_m1_, d_m2_; AttnW d_at_;
  std::vector<std::vector<ResW>> d_blk_; std::vector<ConvW*> d_up_; GNW d_no_; ConvW* d_out_ = nullptr;
  int in_ch_, out_ch_, embed_, moments_;
};

VAEKL::VAEKL(const cd_net_desc& d) {
  desc = d;
  // round 5: the first stage in the reference's arithmetic too (`precision = "full"` covers the VAE,
  // stable_diffusion_stochastic_text_wrapper.py:117, autoencoder.py:324-333): CD_PREC_F32 runs every layer on the fp32
  // path (f32_path.hip), CD_PREC_F32X3 runs the GroupNorm-fed convolutions - 97 % of the FLOPs - as three-term split-fp16
  // products and the rest (nin_shortcut, down / up-sampling convs on raw activations, the single-head attention) in fp32
  set_precision(d);
  CD_CHECK(!(f32 && d.n_embed > 0), "the VQ first stage (codebook lookup on 16-bit rows) runs in the 16-bit format only");
  ch_ = d.model_channels; nres_ = d.num_res_blocks; nlev_ = d.n_mult;
  for (int i = 0; i < nlev_; ++i) mult_.push_back(d.channel_mult[i]);
  z_channels = d.z_channels; embed_ = d.embed_dim; in_ch_ = d.in_channels; out_ch_ = d.out_channels;
  factor = 1 << (nlev_ - 1);
  // AutoencoderKL: double_z, Gaussian posterior (autoencoder.py:285-333). VQModelInterface (n_embed > 0): the encoder
  // emits z_channels directly and decode() snaps to the codebook first (autoencoder.py:264-282)
  CD_CHECK((d.double_z != 0) != (d.n_embed > 0), "first stage must be either KL (double_z) or VQ (n_embed > 0)");
  CD_CHECK(d.n_attn == 0, "attn_resolutions inside the VAE levels are not used by the f4 / f8 configs");
  const int zmul = d.double_z ? 2 : 1;
  moments_ = zmul * z_channels;
  moments_channels = zmul * embed_;
  n_embed = d.n_embed;
  // ---- encoder (model.py:368-459)
  e_in_ = make_conv(params, "encoder.conv_in", ch_, in_ch_, 3);
  int bin = ch_;
  e_blk_.resize(nlev_); e_down_.assign(nlev_, nullptr);
  for (int l = 0; l < nlev_; ++l) {
    const int bout = ch_ * mult_[l];
    for (int b = 0; b < nres_; ++b) {
      e_blk_[l].push_back(mk_res(params, "encoder.down." + std::to_string(l) + ".block." + std::to_string(b), bin, bout));
      bin = bout;
    }
    if (l != nlev_ - 1) e_down_[l] = make_conv(params, "encoder.down." + std::to_string(l) + ".downsample.conv", bin, bin, 3);
  }
  e_m1_ = mk_res(params, "encoder.mid.block_1", bin, bin);
  e_at_ = mk_at(params, "encoder.mid.attn_1", bin);
  e_m2_ = mk_res(params, "encoder.mid.block_2", bin, bin);
  e_no_ = make_gn(params, "encoder.norm_out", bin, kGnEps);
  e_out_ = make_conv(params, "encoder.conv_out", moments_, bin, 3);
  quant_ = make_conv(params, "quant_conv", zmul * embed_, moments_, 1);
  if (n_embed > 0) {
    float* cb = params.new_vec(n_embed * embed_);
    params.mat_f32("quantize.embedding.weight", cb, n_embed, embed_);
    codebook = cb;
  }
  // ---- decoder (model.py:462-568)
  pq_ = make_conv(params, "post_quant_conv", z_channels, embed_, 1);
  bin = ch_ * mult_[nlev_ - 1];
  d_in_ = make_conv(params, "decoder.conv_in", bin, z_channels, 3);
  d_m1_ = mk_res(params, "decoder.mid.block_1", bin, bin);
  d_at_ = mk_at(params, "decoder.mid.attn_1", bin);
  d_m2_ = mk_res(params, "decoder.mid.block_2", bin, bin);
  d_blk_.resize(nlev_); d_up_.assign(nlev_, nullptr);
  for (int l = nlev_ - 1; l >= 0; --l) {
    const int bout = ch_ * mult_[l];
    for (int b = 0; b <= nres_; ++b) {
      d_blk_[l].push_back(mk_res(params, "decoder.up." + std::to_string(l) + ".block." + std::to_string(b), bin, bout));
      bin = bout;
    }
    if (l != 0) d_up_[l] = make_conv(params, "decoder.up." + std::to_string(l) + ".upsample.conv", bin, bin, 3);
  }
  d_no_ = make_gn(params, "decoder.norm_out", bin, kGnEps);
  d_out_ = make_conv(params, "decoder.conv_out", out_ch_, bin, 3);
}

void VAEKL::encode_moments(Ctx& c, const bf16_t* img, int B, int H, int W, float* moments) {
  const size_t mk = c.arena->mark();
  PrecisionScope prec(c, f32, x3);
  const size_t esz = f32 ? 4 : 2;
  const Act x = net_input_act(img, B, H, W, round_up(in_ch_, 32), f32, x3);
  ConvOpts o3; o3.want_stats = true;
  Act h = conv_fwd(c, *e_in_, x, nullptr, o3);
  for (int l = 0; l < nlev_; ++l) {
    for (auto& r : e_blk_[l]) h = res_fwd(c, r, h, nullptr, nullptr, 0, true);
    if (e_down_[l]) { ConvOpts od; od.stride = 2; od.asym = true; od.want_stats = true; h = conv_fwd(c, *e_down_[l], h, nullptr, od); }
  }
  h = res_fwd(c, e_m1_, h, nullptr, nullptr, 0, true);
  h = attn_block_fwd(c, e_at_, h);
  h = res_fwd(c, e_m2_, h, nullptr, nullptr, 0, true);
  Act n = groupnorm_fwd(c, e_no_, h, nullptr, true);
  // conv_out -> bf16 padded to 32 channels so the 1x1 quant_conv can consume it
  const int cp = round_up(moments_, 32);
  Act mo = alloc_act(c, B, h.H, h.W, cp);
  HIP_CHECK(hipMemsetAsync(mo.p, 0, (size_t)mo.rows() * cp * esz, c.st));
  ConvOpts oo; oo.out = mo.p; oo.out_ld = cp;
  conv_fwd(c, *e_out_, n, nullptr, oo);
  ConvOpts oq; oq.pad = 0; oq.out_f32 = true; oq.out = moments; oq.out_ld = moments_channels;
  conv_fwd(c, *quant_, mo, nullptr, oq);
  c.arena->release(mk);
}

void VAEKL::decode(Ctx& c, const bf16_t* z, int B, int hl, int wl, float* img) {
  const size_t mk = c.arena->mark();
  PrecisionScope prec(c, f32, x3);
  const Act x = net_input_act(z, B, hl, wl, round_up(embed_, 32), f32, x3);
  const int cp = round_up(z_channels, 32);
  Act zq = alloc_act(c, B, hl, wl, cp);
  HIP_CHECK(hipMemsetAsync(zq.p, 0, (size_t)zq.rows() * cp * (f32 ? 4 : 2), c.st));
  ConvOpts oq; oq.pad = 0; oq.out = zq.p; oq.out_ld = cp;
  conv_fwd(c, *pq_, x, nullptr, oq);
  ConvOpts o3; o3.want_stats = true;
  Act h = conv_fwd(c, *d_in_, zq, nullptr, o3);
  h = res_fwd(c, d_m1_, h, nullptr, nullptr, 0, true);
  h = attn_block_fwd(c, d_at_, h);
  h = res_fwd(c, d_m2_, h, nullptr, nullptr, 0, true);
  for (int l = nlev_ - 1; l >= 0; --l) {
    for (auto& r : d_blk_[l]) h = res_fwd(c, r, h, nullptr, nullptr, 0, true);
    if (d_up_[l]) { ConvOpts ou; ou.up = true; ou.want_stats = true; h = conv_fwd(c, *d_up_[l], h, nullptr, ou); }
  }
  Act n = groupnorm_fwd(c, d_no_, h, nullptr, true);
  ConvOpts oo; oo.out_f32 = true; oo.out = img; oo.out_ld = out_ch_;
  conv_fwd(c, *d_out_, n, nullptr, oo);
  c.arena->release(mk);
}

// ================================================================== Ho et al. DDPM U-Net
class UNetHo : public UNet {
 public:
  explicit UNetHo(const cd_net_desc& d);
  int kind() const override { return CD_NET_UNET_HO; }
  void forward(Ctx& c, const UNetIO& io) override;
  size_t workspace_hint(int B) const override {
    return (size_t)B * image_size * image_size * ch_ * 8 * 2 * 24 + (64u << 20);
  }
 private:
  int ch_, nres_, nlev_, temb_ch_;
  std::vector<int> mult_;
  TimeEmb te_;
  ConvW* cin_ = nullptr;
  struct Lvl { std::vector<ResW> blk; std::vector<AttnW> att; ConvW* resamp = nullptr; };
  std::vector<Lvl> down_, up_;
  ResW m1_, m2_; AttnW mat_;
  GNW no_; ConvW* cout_ = nullptr;
};

UNetHo::UNetHo(const cd_net_desc& d) {
  desc = d;
  set_precision(d);
  ch_ = d.model_channels; nres_ = d.num_res_blocks; nlev_ = d.n_mult; temb_ch_ = 4 * ch_;
  image_size = d.image_size; out_channels = d.out_channels; in_cpad = round_up(d.in_channels, 32);
  CD_CHECK(ch_ % 32 == 0, "ch must be a multiple of 32");
  CD_CHECK(d.conv_resample, "resamp_with_conv=False is not used by the reference configs");
  for (int i = 0; i < nlev_; ++i) mult_.push_back(d.channel_mult[i]);
  auto has_attn = [&](int res) { for (int i = 0; i < d.n_attn; ++i) if (d.attn[i] == res) return true; return false; };
  std::vector<std::pair<std::string, ResW*>> temb_users;
  cin_ = make_conv(params, "conv_in", ch_, d.in_channels, 3);
  int res = d.image_size, bin = ch_;
  std::vector<int> in_mult{1};
  for (int m : mult_) in_mult.push_back(m);
  down_.resize(nlev_);
  for (int l = 0; l < nlev_; ++l) {
    bin = ch_ * in_mult[l];
    const int bout = ch_ * mult_[l];
    down_[l].blk.reserve(nres_); down_[l].att.reserve(nres_);
    for (int b = 0; b < nres_; ++b) {
      const std::string pfx = "down." + std::to_string(l);
      down_[l].blk.push_back(mk_res(params, pfx + ".block." + std::to_string(b), bin, bout));
      temb_users.push_back({pfx + ".block." + std::to_string(b), &down_[l].blk.back()});
      bin = bout;
      if (has_attn(res)) down_[l].att.push_back(mk_at(params, pfx + ".attn." + std::to_string(b), bin));
    }
    if (l != nlev_ - 1) {
      down_[l].resamp = make_conv(params, "down." + std::to_string(l) + ".downsample.conv", bin, bin, 3);
      res /= 2;
    }
  }
  m1_ = mk_res(params, "mid.block_1", bin, bin); temb_users.push_back({"mid.block_1", &m1_});
  mat_ = mk_at(params, "mid.attn_1", bin);
  m2_ = mk_res(params, "mid.block_2", bin, bin); temb_users.push_back({"mid.block_2", &m2_});
  up_.resize(nlev_);
  for (int l = nlev_ - 1; l >= 0; --l) {
    const int bout = ch_ * mult_[l];
    int skip_in = ch_ * mult_[l];
    up_[l].blk.reserve(nres_ + 1); up_[l].att.reserve(nres_ + 1);
    for (int b = 0; b <= nres_; ++b) {
      if (b == nres_) skip_in = ch_ * in_mult[l];
      const std::string pfx = "up." + std::to_string(l);
      up_[l].blk.push_back(mk_res(params, pfx + ".block." + std::to_string(b), bin + skip_in, bout));
      temb_users.push_back({pfx + ".block." + std::to_string(b), &up_[l].blk.back()});
      bin = bout;
      if (has_attn(res)) up_[l].att.push_back(mk_at(params, pfx + ".attn." + std::to_string(b), bin));
    }
    if (l != 0) {
      up_[l].resamp = make_conv(params, "up." + std::to_string(l) + ".upsample.conv", bin, bin, 3);
      res *= 2;
    }
  }
  no_ = make_gn(params, "norm_out", bin, kGnEps);
  cout_ = make_conv(params, "conv_out", d.out_channels, bin, 3);
  // timestep embedding (diffusion.py:210-217, 294-297) + fused temb_proj of every ResnetBlock
  te_.mode = 1; te_.dim = ch_; te_.hidden = temb_ch_;
  te_.w0 = params.new_vec(temb_ch_ * ch_); te_.b0 = params.new_vec(temb_ch_);
  te_.w1 = params.new_vec(temb_ch_ * temb_ch_); te_.b1 = params.new_vec(temb_ch_);
  params.mat_f32("temb.dense.0.weight", te_.w0, temb_ch_, ch_);
  params.vec("temb.dense.0.bias", te_.b0, temb_ch_);
  params.mat_f32("temb.dense.1.weight", te_.w1, temb_ch_, temb_ch_);
  params.vec("temb.dense.1.bias", te_.b1, temb_ch_);
  int total = 0;
  for (auto& u : temb_users) { u.second->emb_off = total; total += u.second->cout; }
  te_.proj_total = total;
  te_.proj_w = params.new_vec(total * temb_ch_);
  te_.proj_b = params.new_vec(total);
  for (auto& u : temb_users) {
    params.mat_f32(u.first + ".temb_proj.weight", te_.proj_w, u.second->cout, temb_ch_, u.second->emb_off);
    params.bias_rows(u.first + ".temb_proj.bias", u.second->cout, te_.proj_b, u.second->emb_off, u.second->cout, 0,
                     u.second->cout, 0);
  }
}

void UNetHo::forward(Ctx& c, const UNetIO& io) {
  const size_t mk0 = c.arena->mark();
  PrecisionScope prec(c, f32, x3);
  const int R = image_size;
  const float* proj = time_emb_fwd(c, te_, io);
  const int pl = te_.proj_total;
  const Act x = net_input_act(io.xin, io.B, R, R, in_cpad, f32, x3);
  ConvOpts o3; o3.want_stats = true;
  std::vector<Act> hs;
  hs.push_back(conv_fwd(c, *cin_, x, nullptr, o3));
  for (int l = 0; l < nlev_; ++l) {
    for (int b = 0; b < nres_; ++b) {
      Act h = res_fwd(c, down_[l].blk[b], hs.back(), nullptr, proj, pl, io.t_shared);
      if (!down_[l].att.empty()) h = attn_block_fwd(c, down_[l].att[b], h);
      hs.push_back(h);
    }
    if (down_[l].resamp) {
      ConvOpts od; od.stride = 2; od.asym = true; od.want_stats = true;
      hs.push_back(conv_fwd(c, *down_[l].resamp, hs.back(), nullptr, od));
    }
  }
  Act h = hs.back();
  h = res_fwd(c, m1_, h, nullptr, proj, pl, io.t_shared);
  h = attn_block_fwd(c, mat_, h);
  h = res_fwd(c, m2_, h, nullptr, proj, pl, io.t_shared);
  for (int l = nlev_ - 1; l >= 0; --l) {
    for (int b = 0; b <= nres_; ++b) {
      Act skip = hs.back(); hs.pop_back();
      h = res_fwd(c, up_[l].blk[b], h, &skip, proj, pl, io.t_shared);
      if (!up_[l].att.empty()) h = attn_block_fwd(c, up_[l].att[b], h);
    }
    if (up_[l].resamp) { ConvOpts ou; ou.up = true; ou.want_stats = true; h = conv_fwd(c, *up_[l].resamp, h, nullptr, ou); }
  }
  Act n = groupnorm_fwd(c, no_, h, nullptr, true);
  ConvOpts oo; oo.out_f32 = true; oo.out = io.out; oo.out_ld = io.out_ld;
  conv_fwd(c, *cout_, n, nullptr, oo);
  c.arena->release(mk0);
}

}  // namespace

std::unique_ptr<VAE> make_vae_kl(const cd_net_desc& d) { return std::unique_ptr<VAE>(new VAEKL(d)); }
std::unique_ptr<UNet> make_unet_ho(const cd_net_desc& d) { return std::unique_ptr<UNet>(new UNetHo(d)); }

}  // namespace cd

// Network engine implementation (see engine.h).
//
// Topology enumeration restates the reference constructors (openaimodel.py:528-707 UNetModel,
// :824-929 EncoderUNetModel) so that the parameter table equals the reference state_dict() order;
// the forward schedule restates UNetModel.forward (:731-768) / EncoderUNetModel.forward (:969-991) as a
// fixed list of kernel launches on one HIP stream, with
//   * skip-concat and nearest-x2 upsample folded into the consumer's A-tile loader (never materialised),
//   * GroupNorm+SiLU folded into the consumer conv, statistics cached per tensor,
//   * all ResBlock emb_layers of the network evaluated by ONE linear launch per forward.
#include "engine.h"

#include <algorithm>
#include <atomic>
#include <deque>
#include <mutex>

namespace drm {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }

const DeviceInfo* device_info() {
  constexpr int MAX_DEV = 64;
  static DeviceInfo info[MAX_DEV];
  static std::atomic<int> state[MAX_DEV];  // 0 unknown, 1 valid, 2 rejected (zero-initialised)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) {
    set_error("device_info: no current HIP device");
    return nullptr;
  }
  int st = state[dev].load(std::memory_order_acquire);
  if (st == 0) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    st = state[dev].load(std::memory_order_acquire);
    if (st == 0) {
      hipDeviceProp_t p;
      if (hipGetDeviceProperties(&p, dev) != hipSuccess) {
        set_error("device_info: hipGetDeviceProperties failed");
        return nullptr;
      }
      DeviceInfo d;
      d.ordinal = dev;
      d.cus = p.multiProcessorCount;
      d.lds_per_cu = p.maxSharedMemoryPerMultiProcessor;
      const std::string arch = p.gcnArchName;
      // XCD count is not a device property: it is 8 on the one part this library targets (gfx950 with 256 CUs)
      d.xcds = (arch.rfind("gfx950", 0) == 0 && d.cus == 256) ? 8 : 0;
      info[dev] = d;
      st = (d.xcds == 8 && d.lds_per_cu >= 160 * 1024) ? 1 : 2;
      state[dev].store(st, std::memory_order_release);
    }
  }
  if (st != 1) {
    set_error("unsupported device " + std::to_string(dev) + ": libdrmnet_hip is built for MI355X (gfx950, 256 CUs in 8 XCDs, 160 KiB LDS per CU); found " +
              std::to_string(info[dev].cus) + " CUs, " + std::to_string(info[dev].lds_per_cu) + " B LDS per CU");
    return nullptr;
  }
  return &info[dev];
}

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

UNet::~UNet() {
  for (float* w : wsets)
    if (w) (void)hipFree(w);
}

size_t ParamTable::reserve(size_t floats) {
  const size_t at = wbuf_floats;
  wbuf_floats += (floats + 63) & ~size_t(63);
  return at;
}

size_t ParamTable::add_copy(const std::string& name, std::vector<int64_t> shape, size_t padded_count) {
  ParamSlot p;
  p.name = name;
  p.shape = shape;
  p.kind = PK_COPY;
  size_t cnt = 1;
  for (auto v : shape) cnt *= (size_t)v;
  p.count = cnt;
  p.dst = reserve(std::max(cnt, padded_count));
  params.push_back(p);
  return p.dst;
}

size_t ParamTable::add_conv(const std::string& name, int cout, int cin, int k, int coutp, int cinp, bool conv1d, size_t* scale_off, bool mx_site) {
  ParamSlot p;
  p.name = name;
  if (conv1d) p.shape = {cout, cin, k};
  else p.shape = {cout, cin, k, k};
  p.kind = PK_CONV;
  p.cout = cout; p.cin = cin; p.taps = conv1d ? k : k * k; p.coutp = coutp; p.cinp = cinp;
  p.mx_site = mx_site;
  p.dst = reserve(packed_conv_weight_floats(p.taps, coutp, cinp));
  p.scale_dst = reserve(64);
  if (scale_off) *scale_off = p.scale_dst;
  params.push_back(p);
  return p.dst;
}

void ParamTable::add_res(Layer& l, const std::string& px, int cin, int cout, int up_c0) {
  l.kind = Layer::RES;
  ResLayer& r = l.res;
  r.cin = cin; r.cout = cout; r.has_skip = (cin != cout);
  r.n1_w = add_copy(px + ".in_layers.0.weight", {cin});
  r.n1_b = add_copy(px + ".in_layers.0.bias", {cin});
  r.c1_w = add_conv(px + ".in_layers.2.weight", cout, cin, 3, cout, cin, false, &r.c1_s, true);
  if (upconv_split_packable(up_c0, cin - up_c0, cout)) {  // (same tensor, two more images: the parameter table does not change)
    ParamSlot& p = params.back();
    p.up_c0 = r.up_c0 = up_c0;
    p.upa_dst = r.c1a_w = reserve(packed_conv_weight_floats(4, 4 * cout, up_c0));
    p.upa_scale = r.c1a_s = reserve(64);
    p.upb_dst = r.c1b_w = reserve(packed_conv_weight_floats(9, cout, cin - up_c0));
    p.upb_scale = r.c1b_s = reserve(64);
  }
  r.c1_b = add_copy(px + ".in_layers.2.bias", {cout});
  r.emb_off = emb_total;
  emb_total += cout;
  // emb_layers.1.{weight,bias}: destinations are fixed up by finish(), once emb_total is known (fused [sum Cout][emb_dim] matrix)
  ParamSlot ew; ew.name = px + ".emb_layers.1.weight"; ew.shape = {cout, emb_dim}; ew.kind = PK_COPY; ew.count = (size_t)cout * emb_dim; ew.dst = (size_t)-1; ew.cout = r.emb_off;
  params.push_back(ew);
  ParamSlot eb; eb.name = px + ".emb_layers.1.bias"; eb.shape = {cout}; eb.kind = PK_COPY; eb.count = (size_t)cout; eb.dst = (size_t)-2; eb.cout = r.emb_off;
  params.push_back(eb);
  r.n2_w = add_copy(px + ".out_layers.0.weight", {cout});
  r.n2_b = add_copy(px + ".out_layers.0.bias", {cout});
  r.c2_w = add_conv(px + ".out_layers.3.weight", cout, cout, 3, cout, cout, false, &r.c2_s, true);
  r.c2_b = add_copy(px + ".out_layers.3.bias", {cout});
  if (r.has_skip) {
    r.sk_w = add_conv(px + ".skip_connection.weight", cout, cin, 1, cout, cin, false, &r.sk_s);
    r.sk_b = add_copy(px + ".skip_connection.bias", {cout});
  }
}

void ParamTable::add_attn(Layer& l, const std::string& px, int ch) {
  l.kind = Layer::ATTN;
  AttnLayer& a = l.attn;
  a.ch = ch;
  a.n_w = add_copy(px + ".norm.weight", {ch});
  a.n_b = add_copy(px + ".norm.bias", {ch});
  // proj_out is folded into the v rows of qkv when a parameter set is packed (pack(): launch_fold_attn_params over these four tensors); the
  // manifest keeps all of them, the packed buffer only the folded qkv
  a.qkv_w = add_conv(px + ".qkv.weight", 3 * ch, ch, 1, 3 * ch, ch, true, &a.qkv_s);
  params.back().attn_fold = true;
  a.qkv_b = add_copy(px + ".qkv.bias", {3 * ch});
  params.back().kind = PK_FOLDED;
  ParamSlot pw; pw.name = px + ".proj_out.weight"; pw.shape = {ch, ch, 1}; pw.kind = PK_FOLDED; pw.count = (size_t)ch * ch;
  params.push_back(pw);
  ParamSlot pb; pb.name = px + ".proj_out.bias"; pb.shape = {ch}; pb.kind = PK_FOLDED; pb.count = (size_t)ch;
  params.push_back(pb);
}

int UNet::build(const drm_unet_desc& d) {
  desc = d;
  DRM_REQUIRE(d.kind == 0 || d.kind == 1, "kind must be 0 (UNetModel) or 1 (EncoderUNetModel)");
  DRM_REQUIRE(d.n_levels >= 1 && d.n_levels <= DRM_MAX_LEVELS, "n_levels");
  DRM_REQUIRE(d.n_attn >= 0 && d.n_attn <= DRM_MAX_LEVELS, "n_attn");
  DRM_REQUIRE(d.model_channels > 0 && d.model_channels % 32 == 0, "model_channels must be a multiple of 32 (GroupNorm32)");
  DRM_REQUIRE(d.in_channels > 0 && d.in_channels <= 32, "in_channels");
  DRM_REQUIRE(d.out_channels > 0 && d.out_channels <= 32, "out_channels");
  DRM_REQUIRE(d.num_res_blocks >= 1, "num_res_blocks");
  const int mc = d.model_channels;
  emb_dim = 4 * mc;
  DRM_REQUIRE(emb_dim <= 512, "time_embed_dim (4*model_channels) must be <= 512");
  in_cp = round_up(d.in_channels, 32);  // one 32-channel K chunk: the stem runs on the same kernels as every other conv
  out_cp = 32;
  auto has_attn = [&](int ds) {
    for (int i = 0; i < d.n_attn; ++i)
      if (d.attention_resolutions[i] == ds) return true;
    return false;
  };

  te0_w = add_copy("time_embed.0.weight", {emb_dim, mc});
  te0_b = add_copy("time_embed.0.bias", {emb_dim});
  te2_w = add_copy("time_embed.2.weight", {emb_dim, emb_dim});
  te2_b = add_copy("time_embed.2.bias", {emb_dim});
  stem_w = add_conv("input_blocks.0.0.weight", mc, d.in_channels, 3, mc, in_cp, false, &stem_s);
  stem_param = (int)params.size() - 1;
  stem_b = add_copy("input_blocks.0.0.bias", {mc});
  input_blocks.emplace_back();

  std::vector<int> chans{mc};
  int ch = mc, ds = 1, idx = 1;
  for (int level = 0; level < d.n_levels; ++level) {
    const int m = d.channel_mult[level];
    DRM_REQUIRE(m >= 1, "channel_mult");
    for (int k = 0; k < d.num_res_blocks; ++k) {
      std::vector<Layer> ls(1);
      add_res(ls[0], "input_blocks." + std::to_string(idx) + ".0", ch, m * mc);
      ch = m * mc;
      if (has_attn(ds)) {
        ls.emplace_back();
        add_attn(ls.back(), "input_blocks." + std::to_string(idx) + ".1", ch);
      }
      input_blocks.push_back(ls);
      chans.push_back(ch);
      ++idx;
    }
    if (level != d.n_levels - 1) {
      std::vector<Layer> ls(1);
      ls[0].kind = Layer::DOWN;
      input_blocks.push_back(ls);
      chans.push_back(ch);
      ++idx;
      ds *= 2;
    }
  }
  middle.resize(3);
  add_res(middle[0], "middle_block.0", ch, ch);
  add_attn(middle[1], "middle_block.1", ch);
  add_res(middle[2], "middle_block.2", ch, ch);
  if (d.kind == 0) {
    int oidx = 0;
    bool up_in = false;  // the block's input h arrives through an Upsample
    for (int level = d.n_levels - 1; level >= 0; --level) {
      const int m = d.channel_mult[level];
      for (int i = 0; i <= d.num_res_blocks; ++i) {
        const int ich = chans.back();
        chans.pop_back();
        std::vector<Layer> ls(1);
        add_res(ls[0], "output_blocks." + std::to_string(oidx) + ".0", ch + ich, mc * m, up_in ? ch : 0);
        up_in = false;
        ch = mc * m;
        if (has_attn(ds)) {
          ls.emplace_back();
          add_attn(ls.back(), "output_blocks." + std::to_string(oidx) + ".1", ch);
        }
        if (level && i == d.num_res_blocks) {
          ls.emplace_back();
          ls.back().kind = Layer::UP;
          up_in = true;
          ds /= 2;
        }
        output_blocks.push_back(ls);
        ++oidx;
      }
    }
  }
  final_ch = ch;
  on_w = add_copy("out.0.weight", {ch});
  on_b = add_copy("out.0.bias", {ch});
  if (d.kind == 0) {
    DRM_REQUIRE(ch == mc, "UNetModel head expects model_channels inputs");
    oc_w = add_conv("out.2.weight", d.out_channels, mc, 3, out_cp, mc, false, &oc_s);
    oc_b = add_copy("out.2.bias", {d.out_channels}, out_cp);
  } else {
    oc_w = add_copy("out.3.weight", {d.out_channels, ch, 1, 1});
    oc_b = add_copy("out.3.bias", {d.out_channels});
  }
  if (stem_direct_applicable(d.in_channels, mc)) stem_direct_w = (long long)reserve(stem_weight_floats());
  finish();
  return DRM_OK;
}

void ParamTable::finish() {
  scratch_off = reserve(64);
  // fused embedding projection
  embcat_w = reserve((size_t)emb_total * emb_dim);
  embcat_b = reserve((size_t)emb_total);
  for (auto& p : params) {
    if (p.dst == (size_t)-1) p.dst = embcat_w + (size_t)p.cout * emb_dim;
    else if (p.dst == (size_t)-2) p.dst = embcat_b + (size_t)p.cout;
  }
}

int pack_conv_image(int precision, const float* w, float* packed, float* scale, unsigned* scratch, int Cout, int Cin, int taps, int CoutP, int CinP,
                    bool mx_site, hipStream_t s) {
  if (conv_split_weights(precision, CinP))
    return launch_pack_conv_weight_split(w, packed, scale, scratch, Cout, Cin, taps, CoutP, CinP, s, precision == PREC_F16MX && mx_site,
                                         precision == PREC_BF16);
  return launch_pack_conv_weight(w, packed, Cout, Cin, taps, CoutP, CinP, s);
}

// the widest of: the folded attention parameters ([3C][C] weight + [3C] bias), the two raw weight tensors an upsampled-input in_layers conv is
// split into (launch_fold_upconv_weight)
size_t ParamTable::staging_floats() const {
  size_t n = 0;
  for (const ParamSlot& p : params) {
    if (p.attn_fold) n = std::max(n, (size_t)p.cout * p.cin + (size_t)p.cout);
    if (p.up_c0) n = std::max(n, (size_t)16 * p.cout * p.up_c0 + (size_t)9 * p.cout * (p.cin - p.up_c0));
  }
  return n;
}

int ParamTable::pack(const float* const* ptrs, int count, float* wbuf, int precision, float* staging, hipStream_t s) const {
  DRM_REQUIRE(count == (int)params.size(), "parameter count mismatch: got " + std::to_string(count) + ", expected " + std::to_string(params.size()));
  DRM_HIP_CHECK(hipMemsetAsync(wbuf, 0, wbuf_floats * sizeof(float), s));
  auto conv = [&](const float* w, size_t dst, size_t scale_dst, int cout, int cin, int taps, int coutp, int cinp, bool mx_site) -> int {
    return pack_conv_image(precision, w, wbuf + dst, wbuf + scale_dst, reinterpret_cast<unsigned*>(wbuf + scratch_off), cout, cin, taps, coutp, cinp,
                           mx_site, s);
  };
  for (size_t i = 0; i < params.size(); ++i) {
    const ParamSlot& p = params[i];
    DRM_REQUIRE(ptrs[i] != nullptr, "null parameter pointer for " + p.name);
    if (p.kind == PK_FOLDED) continue;  // (consumed at the block's qkv.weight slot)
    const float* w = ptrs[i];
    if (p.attn_fold) {
      DRM_REQUIRE(i + 3 < params.size() && ptrs[i + 1] && ptrs[i + 2] && ptrs[i + 3], "attention block parameters of " + p.name);
      float* fb = staging + (size_t)p.cout * p.cin;
      DRM_TRY(launch_fold_attn_params(ptrs[i], ptrs[i + 1], ptrs[i + 2], ptrs[i + 3], staging, fb, p.cin, s));
      DRM_HIP_CHECK(hipMemcpyAsync(wbuf + params[i + 1].dst, fb, (size_t)p.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
      w = staging;
    }
    if (p.kind == PK_COPY) {
      DRM_HIP_CHECK(hipMemcpyAsync(wbuf + p.dst, w, p.count * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else {
      DRM_TRY(conv(w, p.dst, p.scale_dst, p.cout, p.cin, p.taps, p.coutp, p.cinp, p.mx_site));
      if (p.up_c0) {  // each image with its own pre-scaling: the folded taps are sums of up to four weights
        const int c0 = p.up_c0, c1 = p.cin - p.up_c0;
        float* wa = staging;
        float* wb = staging + (size_t)16 * p.cout * c0;
        DRM_TRY(launch_fold_upconv_weight(w, wa, wb, p.cout, c0, c1, s));
        DRM_TRY(conv(wa, p.upa_dst, p.upa_scale, 4 * p.cout, c0, 4, 4 * p.cout, c0, p.mx_site));
        DRM_TRY(conv(wb, p.upb_dst, p.upb_scale, p.cout, c1, 9, p.cout, c1, p.mx_site));
      }
    }
  }
  return DRM_OK;
}

int UNet::load(const float* const* ptrs, int count, hipStream_t s, int set) {
  DRM_REQUIRE(set >= 0 && set < NSETS, "weight set index");
  if (!wsets[set]) DRM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&wsets[set]), wbuf_floats * sizeof(float)));
  float* wbuf = wsets[set];
  loaded[set] = false;
  Scratch staging(s);  // (freed when the last pack has run)
  if (staging_floats()) DRM_TRY(staging.reserve(staging_floats() * sizeof(float)));
  DRM_TRY(pack(ptrs, count, wbuf, precision, static_cast<float*>(staging.p), s));
  if (stem_direct_w >= 0) DRM_TRY(launch_pack_stem_weight(ptrs[stem_param], wbuf + stem_direct_w, desc.model_channels, desc.in_channels, precision == PREC_FP32, s));
  loaded[set] = true;
  loaded_precision[set] = precision;
  return DRM_OK;
}

// ------------------------------------------------------------------------------------------------ blocks

Act new_act(Ctx& c, int C, int H, int W) {
  Act a;
  a.C = C; a.H = H; a.W = W;
  a.p = c.ar->alloc<float>((size_t)c.N * H * W * C);
  a.mom = reinterpret_cast<double2*>(c.ar->alloc_stats((size_t)c.N * C * sizeof(double2), &a.mom_zeroed));
  return a;
}

int ensure_moments(Ctx& c, Act& a) {
  if (a.mom_valid) return DRM_OK;
  const int hs = a.H >> a.up, ws = a.W >> a.up;
  const size_t m = c.ar->mark();
  const int splits = chan_moments_splits(hs * ws, a.C);
  double* partial = c.ar->alloc<double>((size_t)c.N * splits * a.C * 2);
  if (!c.dry()) DRM_TRY(launch_chan_moments(a.p, c.N, hs * ws, a.C, partial, a.mom, c.s));
  c.ar->release(m);
  a.mom_valid = true;
  return DRM_OK;
}

int expect_raw_sums(Ctx& c, Act& a) {
  if (!c.dry() && !a.mom_zeroed) DRM_HIP_CHECK(hipMemsetAsync(a.mom, 0, (size_t)c.N * a.C * sizeof(double2), c.s));
  a.mom_valid = true;
  a.mom_sums = true;
  return DRM_OK;
}

// a.ksplit of the plan and, for a split-K plan, its workspace (allocated in sizing and real passes alike): a.split_stride, the slabs at
// a.split_ws and, for the in-launch finish, the zeroed arrival counters at a.tile_ticket -- from the pass's statistics pool, else zeroed here
static void splitk_workspace(Ctx& c, ConvArgs& a, const ConvPlan& p) {
  a.ksplit = p.ksplit;
  if (p.ksplit <= 1) return;
  a.split_stride = (size_t)a.N * a.H * a.W * a.Cout;
  if (p.finish == SPLIT_IN_LAUNCH) {
    bool zeroed = false;
    a.tile_ticket = reinterpret_cast<unsigned*>(c.ar->alloc_stats(p.tickets * sizeof(unsigned), &zeroed));
    if (!zeroed && !c.dry()) (void)hipMemsetAsync(a.tile_ticket, 0, p.tickets * sizeof(unsigned), c.s);
  }
  a.split_ws = c.ar->alloc<float>(a.split_stride * a.ksplit);
}

int run_conv(Ctx& c, ConvArgs& a, const ConvPlan& p, const float* Wb, size_t scale_off, Act* stats_for) {
  if (p.kernel == CONV_PIPELINE) {
    a.w_inv_scale = c.split() ? Wb + scale_off + 1 : nullptr;  // (fp32 weights are packed unscaled)
    a.terms = p.terms;
    if (stats_for && !a.out_nchw) {  // (the pipeline accumulates the output's statistics in its epilogue)
      DRM_TRY(expect_raw_sums(c, *stats_for));
      a.stat_out = stats_for->mom;
    }
  }
  return launch_conv(a, p, c.s);
}

// Split-precision convs on an UN-normalised input (skip_connection, stem): stage it through a per-image power of two
// derived from a rigorous bound of max |x| (gn.hip act_pow2_scale_kernel) so nothing saturates or underflows fp16; the factor rides
// on the (scale, shift) tables the staging path applies anyway and is undone per image in the epilogue.  Bound source: the
// per-channel sum-of-squares tables of x0 (channels [lo0, hi0)) and x1, or an absmax word per image.  No-op in fp32 mode.
int raw_input_guard(Ctx& c, ConvArgs& a, const ConvPlan& p, Act* x0, int lo0, int hi0, Act* x1, const unsigned* absmax_bits, int Ctab, int absmax_parts) {
  if (!p.split()) return DRM_OK;
  float* sc = c.ar->alloc<float>((size_t)c.N * Ctab);
  float* sh = c.ar->alloc<float>((size_t)c.N * Ctab);
  float* inv = c.ar->alloc<float>((size_t)c.N);
  if (x0) DRM_TRY(ensure_moments(c, *x0));
  if (x1) DRM_TRY(ensure_moments(c, *x1));
  if (c.dry()) return DRM_OK;
  DRM_TRY(launch_act_pow2_scale(x0 ? x0->mom : nullptr, x0 ? x0->C : 0, lo0, hi0, x0 ? x0->mom_cnt() : 0.0, x1 ? x1->mom : nullptr, x1 ? x1->C : 0,
                                x1 ? x1->mom_cnt() : 0.0, absmax_bits, Ctab, c.N, sc, sh, inv, c.s, absmax_parts));
  a.gn_scale = sc;
  a.gn_shift = sh;
  a.in_inv = inv;
  return DRM_OK;
}

// fold_into: the conv whose plan finalises the tables in its own prologue (ConvPlan::gn_fold: ConvArgs::gnf, gn_fold.h) -- no gn_finalize launch
int gn_params(Ctx& c, Act& x0, Act* x1, const float* gamma, const float* beta, float* scale, float* shift, ConvArgs* guard_for, ConvArgs* fold_into) {
  DRM_TRY(ensure_moments(c, x0));
  if (x1) DRM_TRY(ensure_moments(c, *x1));
  // the same launch can also produce the range-guard tables of a split conv that reads (x0 | x1) un-normalised (skip_connection)
  const int Ctot = x0.C + (x1 ? x1->C : 0);
  float *gs = nullptr, *gh = nullptr, *gi = nullptr;
  if (guard_for) {
    gs = c.ar->alloc<float>((size_t)c.N * Ctot);
    gh = c.ar->alloc<float>((size_t)c.N * Ctot);
    gi = c.ar->alloc<float>((size_t)c.N);
    guard_for->gn_scale = gs;
    guard_for->gn_shift = gh;
    guard_for->in_inv = gi;
  }
  if (c.dry()) return DRM_OK;
  if (fold_into) {
    GnFold& f = fold_into->gnf;
    f.mom0 = x0.mom; f.C0 = x0.C; f.inv0 = x0.mom_inv(); f.cnt0 = x0.mom_cnt();
    f.mom1 = x1 ? x1->mom : nullptr; f.C1 = x1 ? x1->C : 0; f.inv1 = x1 ? x1->mom_inv() : 1.0; f.cnt1 = x1 ? x1->mom_cnt() : 0.0;
    f.gamma = gamma; f.beta = beta; f.scale = scale; f.shift = shift;
    f.guard_scale = gs; f.guard_shift = gh; f.guard_inv = gi;
    return DRM_OK;
  }
  return launch_gn_finalize(x0.mom, x0.C, x0.mom_inv(), x1 ? x1->mom : nullptr, x1 ? x1->C : 0, x1 ? x1->mom_inv() : 1.0, gamma, beta, c.N, scale,
                            shift, c.s, x0.mom_cnt(), x1 ? x1->mom_cnt() : 0.0, gs, gh, gi);
}

// a real pass whose arena ran out hands out null tables: stop before any kernel is launched on them
static int arena_ok(const Ctx& c) {
  if (!c.ar->failed) return DRM_OK;
  set_error("workspace too small: need more than " + std::to_string(c.ar->cap) + " bytes (query drm_unet_workspace_bytes for this shape and precision)");
  return DRM_ERR_WORKSPACE;
}

static std::atomic<int> g_upconv_split{1};
void set_upconv_split(int mode) { g_upconv_split.store(mode); }

// in_layers conv over cat(nearest_x2(x0), x1), by linearity: conv3x3(cat(up(a0), a1)) = PS(conv2x2'(a0)) + conv3x3(a1), a = SiLU(GN(x)) with the
// block's tables (per element: it commutes with the replication).  Launch A: the four parity 2x2 convs on the STORED x0 (taps = 4, Cout' = 4 Cout),
// pixel-shuffled straight into h1; launch B: the ordinary 3x3 conv on x1 with bias, emb, res = out = h1 and the fused output statistics.  A runs 4
// taps where the single launch ran 9 on x0's channels and stages a quarter of the halo pixels.  Takes nothing from the arena or the statistics pool.
// The form runs only where the single launch and both new ones are whole-tile, un-split pipeline launches with no GroupNorm fold (N > 4); the sizing
// pass and the real pass both decide here.
struct UpconvSplit {
  bool on = false;
  ConvArgs a4, b9;  // shape fields
  ConvPlan p4, p9;
};
static UpconvSplit plan_upconv_split(const Ctx& c, const ResLayer& r, const ConvArgs& a, const ConvPlan& pa, const Act& x0, const Act* x1) {
  UpconvSplit u;
  const int mode = g_upconv_split.load(std::memory_order_relaxed);
  if (mode == 0 || !r.up_c0 || !x0.up || !x1 || x0.C != r.up_c0 || !upconv_split_packable(x0.C, x1->C, r.cout)) return u;
  auto plain = [](const ConvPlan& p) { return p.kernel == CONV_PIPELINE && !p.ragged && p.ksplit == 1 && !p.gn_fold && !p.pool; };
  if (!plain(pa)) return u;
  u.a4.C0 = x0.C; u.a4.N = a.N; u.a4.H = a.H >> 1; u.a4.W = a.W >> 1; u.a4.taps = 4; u.a4.Cout = 4 * r.cout; u.a4.mx_site = 1;
  u.b9.C0 = x1->C; u.b9.N = a.N; u.b9.H = a.H; u.b9.W = a.W; u.b9.taps = 9; u.b9.Cout = r.cout; u.b9.mx_site = 1;
  u.p4 = plan_conv(u.a4, c.precision);
  u.p9 = plan_conv(u.b9, c.precision);
  if (!plain(u.p4) || !plain(u.p9)) return u;
  if (r.cout % tile_shape(u.p4.tile).bn() != 0) return u;  // a Cout tile of A lies inside one parity
  // The rule (mode 1).  Measured on the five decoder levels of the batch-32 step, f16mx, single launch -> A + B, two interleaved rounds on one
  // device (profiles/upconv_split_shapes.txt): 128x256 1.755 -> 1.419 ms, 64x128 1.409 -> 1.105, 32x64 0.700 -> 0.544, 16x32 0.310 -> 0.254,
  // round-to-round spread of a shape 0.2 .. 3 %: every level where the form applies wins by 18 .. 22 %, all of them on 256-row tiles at least 128
  // channels wide for A and B alike.  (The 8x16 level is split-K and keeps the single launch.)  Launches on the narrow tiles of sparse grids --
  // small batches, where a launch is a few microseconds and one more launch and epilogue weigh most -- were not measured: they keep the single launch.
  if (mode == 1 && (u.p4.tile > TILE_256x128 || u.p9.tile > TILE_256x128)) return u;
  u.on = true;
  return u;
}

int run_resblock(Ctx& c, const float* Wb, const ResLayer& r, Act& x0, Act* x1, const float* emb_all, int emb_stride, Act& out, Act* pool, bool* pooled) {
  DRM_TRY(arena_ok(c));
  const int H = x0.H, W = x0.W;
  const int C0 = x0.C, C1 = x1 ? x1->C : 0;
  DRM_REQUIRE(C0 + C1 == r.cin, "resblock input channels");
  DRM_REQUIRE(!x1 || (x1->H == H && x1->W == W && !x1->up), "resblock skip tensor shape");
  DRM_REQUIRE(r.has_skip || (!x1 && !x0.up), "identity skip on a concatenated / upsampled input is not supported");
  const size_t mark = c.ar->mark();
  float* sc1 = c.ar->alloc<float>((size_t)c.N * r.cin);
  float* sh1 = c.ar->alloc<float>((size_t)c.N * r.cin);
  Act h1 = new_act(c, r.cout, H, W);
  float* sc2 = c.ar->alloc<float>((size_t)c.N * r.cout);
  float* sh2 = c.ar->alloc<float>((size_t)c.N * r.cout);
  ConvArgs k;  // skip_connection: 1x1 conv on the raw (un-normalised) block input; its range-guard tables come out of the same launch
  ConvArgs a;  // in_layers conv: GroupNorm(x0 | x1) -> SiLU -> 3x3 + emb
  a.src0 = x0.p; a.src1 = x1 ? x1->p : nullptr; a.C0 = C0; a.C1 = C1; a.up0 = x0.up;
  a.N = c.N; a.H = H; a.W = W; a.taps = 9; a.Cout = r.cout; a.mx_site = 1;
  const ConvPlan pa = plan_conv(a, c.precision, false, true);
  ConvPlan pk;
  if (r.has_skip) {
    k.C0 = C0; k.C1 = C1; k.N = c.N; k.H = H; k.W = W; k.taps = 1; k.Cout = r.cout;
    pk = plan_conv(k, c.precision);
  }
  DRM_TRY(gn_params(c, x0, x1, Wb + r.n1_w, Wb + r.n1_b, sc1, sh1, pk.split() ? &k : nullptr, pa.gn_fold ? &a : nullptr));
  splitk_workspace(c, a, pa);
  UpconvSplit up = plan_upconv_split(c, r, a, pa, x0, x1);
  if (up.on) {
    if (!c.dry()) {
      ConvArgs& a4 = up.a4;  // A: the parity 2x2 convs on the stored x0, pixel-shuffled into h1 (weight un-scaling only)
      a4.src0 = x0.p; a4.gn_scale = sc1; a4.gn_shift = sh1; a4.gn_ld = r.cin; a4.silu = 1;
      a4.w = Wb + r.c1a_w; a4.out = h1.p;
      DRM_TRY(run_conv(c, a4, up.p4, Wb, r.c1a_s, nullptr));
      ConvArgs& b9 = up.b9;  // B: 3x3 on the skip tensor + bias + emb + A's result (res = out), statistics of the sum
      b9.src0 = x1->p; b9.gn_scale = sc1 + x0.C; b9.gn_shift = sh1 + x0.C; b9.gn_ld = r.cin; b9.silu = 1;
      b9.w = Wb + r.c1b_w; b9.bias = Wb + r.c1_b;
      b9.emb = emb_all ? emb_all + r.emb_off : nullptr; b9.emb_stride = emb_stride;
      b9.res = h1.p; b9.out = h1.p;
      DRM_TRY(run_conv(c, b9, up.p9, Wb, r.c1b_s, &h1));
    }
  } else if (!c.dry()) {
    a.gn_scale = sc1; a.gn_shift = sh1; a.silu = 1;
    a.w = Wb + r.c1_w; a.bias = Wb + r.c1_b;
    a.emb = emb_all ? emb_all + r.emb_off : nullptr; a.emb_stride = emb_stride;
    a.out = h1.p;
    DRM_TRY(run_conv(c, a, pa, Wb, r.c1_s, &h1));
  }
  ConvArgs b;  // out_layers conv: GroupNorm(h1) -> SiLU -> 3x3 + residual
  b.src0 = h1.p; b.C0 = r.cout; b.N = c.N; b.H = H; b.W = W; b.taps = 9; b.Cout = r.cout; b.mx_site = 1;
  const ConvPlan pb = plan_conv(b, c.precision, pool != nullptr, true);  // (the Downsample behind this block, from this conv's epilogue)
  DRM_TRY(gn_params(c, h1, nullptr, Wb + r.n2_w, Wb + r.n2_b, sc2, sh2, nullptr, pb.gn_fold ? &b : nullptr));
  splitk_workspace(c, b, pb);
  if (pooled) *pooled = pb.pool;
  if (pb.pool) DRM_TRY(expect_raw_sums(c, *pool));
  if (r.has_skip) splitk_workspace(c, k, pk);
  if (!c.dry()) {
    const float* res = x0.p;
    if (r.has_skip) {
      k.src0 = x0.p; k.src1 = x1 ? x1->p : nullptr; k.up0 = x0.up;
      k.w = Wb + r.sk_w; k.bias = Wb + r.sk_b;
      k.out = out.p;
      DRM_TRY(run_conv(c, k, pk, Wb, r.sk_s, nullptr));
      res = out.p;
    }
    b.gn_scale = sc2; b.gn_shift = sh2; b.silu = 1;
    b.w = Wb + r.c2_w; b.bias = Wb + r.c2_b;
    b.res = res; b.out = out.p;
    if (pb.pool) {
      b.pool_out = pool->p;
      b.pool_stat = pool->mom;
    }
    DRM_TRY(run_conv(c, b, pb, Wb, r.c2_s, &out));
  }
  c.ar->release(mark);
  return DRM_OK;
}

// GroupNorm(x) -> qkv 1x1 conv (proj_out folded into its v rows) -> attention core, whose last kernel adds x and leaves out's statistics
int run_attention(Ctx& c, const float* Wb, const AttnLayer& l, Act& x, Act& out) {
  DRM_REQUIRE(!x.up && x.C == l.ch, "attention input");
  DRM_TRY(arena_ok(c));
  const int H = x.H, W = x.W, T = H * W, C = l.ch;
  const size_t mark = c.ar->mark();
  float* sc = c.ar->alloc<float>((size_t)c.N * C);
  float* sh = c.ar->alloc<float>((size_t)c.N * C);
  ConvArgs a;  // qkv: GroupNorm(x) -> 1x1
  a.C0 = C; a.N = c.N; a.H = H; a.W = W; a.taps = 1; a.Cout = 3 * C;
  const ConvPlan pa = plan_conv(a, c.precision, false, true);
  DRM_TRY(gn_params(c, x, nullptr, Wb + l.n_w, Wb + l.n_b, sc, sh, nullptr, pa.gn_fold ? &a : nullptr));
  Act qkv_act = new_act(c, 3 * C, H, W);  // its per-channel sums (fused into the qkv conv's epilogue) bound |q|, |k|, |v| for the split cores
  float* qkv = qkv_act.p;
  const AttnPlan ap = plan_attention(c.N, H, W, C, c.precision);  // which form of the core, and its buffers (attn.hip)
  float* scores = ap.scores_floats ? c.ar->alloc<float>(ap.scores_floats) : nullptr;  // one image group at a time
  // Sizing contract: what drm_*_workspace_bytes answers per network, shape and mode is a recorded table (tests/golden/workspace_bytes.json) that
  // callers size long-lived buffers by.  The fold removed the proj_out stage -- its input tensor, its [N][C] guard table, its split-K slabs and
  // tickets -- and the block still reserves their share of the arena and of the statistics pool, untouched, in the order they were taken, so
  // every recorded answer stands.  (Dropping the reservation means re-recording that table; nothing here reads these bytes.)
  (void)c.ar->alloc<float>((size_t)c.N * T * C);
  const size_t proj_tab = (size_t)c.N * C;
  float* aws = ap.ws_floats ? c.ar->alloc<float>(ap.ws_floats + proj_tab) : nullptr;
  splitk_workspace(c, a, pa);
  {  // (the sizing contract above: the split-K share of a C -> C 1x1 conv on this map)
    ConvArgs p;
    p.C0 = C; p.N = c.N; p.H = H; p.W = W; p.taps = 1; p.Cout = C;
    const ConvPlan pp = plan_conv(p, c.precision);
    if (pp.ksplit > 1) {
      bool zeroed = false;
      if (pp.finish == SPLIT_IN_LAUNCH) (void)c.ar->alloc_stats(pp.tickets * sizeof(unsigned), &zeroed);
      (void)c.ar->alloc<float>((size_t)c.N * T * C * pp.ksplit);
    }
  }
  // (the attention core's last kernel accumulates them; zeroed ahead of the qkv conv: `out` is never `x`, and nothing before that kernel touches out.mom)
  if (ap.out_stats) DRM_TRY(expect_raw_sums(c, out));
  if (!c.dry()) {
    a.src0 = x.p;
    a.gn_scale = sc; a.gn_shift = sh; a.silu = 0;
    a.w = Wb + l.qkv_w; a.bias = Wb + l.qkv_b; a.out = qkv;
    DRM_TRY(run_conv(c, a, pa, Wb, l.qkv_s, &qkv_act));
    DRM_TRY(launch_attention_core(ap, qkv, qkv_act.mom, x.p, scores, out.p, out.mom, aws, c.s));
  }
  c.ar->release(mark);
  if (!ap.out_stats) {  // (the single-kernel form leaves the statistics of its output to the stand-alone moments launch; its partial table takes the
                //  place of the block's temporaries, which are dead in stream order)
    out.mom_valid = false;
    DRM_TRY(ensure_moments(c, out));
  }
  return DRM_OK;
}

// ------------------------------------------------------------------------------------------------ forward

int UNet::dry_forward(int N, int H, int W, Arena& probe) {
  probe.dry = true;
  const int Cx = desc.kind == 0 ? desc.out_channels : desc.in_channels / 2;  // (forward only checks that the two parts sum to in_channels)
  return forward(nullptr, Cx, nullptr, desc.in_channels - Cx, nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, probe, nullptr);
}

int UNet::forward(const float* x, int Cx, const float* cond, int Cc, const int32_t* rows, const float* t_emb, const int64_t* t,
                  const float* tf, float* out, int N, int H, int W, Arena& ar, hipStream_t s) {
  DRM_REQUIRE(ar.dry || loaded[active], "drm_unet_forward before drm_unet_load_params (weight set " + std::to_string(active) + ")");
  DRM_REQUIRE(N > 0, "batch size");
  DRM_REQUIRE(Cx + Cc == desc.in_channels, "x/cond channels must sum to in_channels");
  const int down = 1 << (desc.n_levels - 1);
  // any size the reference's fully convolutional forward accepts (openaimodel.py:731-768): every Downsample must see even sizes
  DRM_REQUIRE(H > 0 && W > 0 && H % down == 0 && W % down == 0,
              "H and W must be multiples of " + std::to_string(down) + " (2^(levels-1): each of the " + std::to_string(desc.n_levels - 1) + " Downsample layers halves the map)");
  const int n_t = (t_emb != nullptr) + (t != nullptr) + (tf != nullptr);
  if (!ar.dry) {
    if (desc.kind == 0) DRM_REQUIRE(n_t == 1, "timesteps and t_emb cannot be specified at the same time");
    else DRM_REQUIRE(n_t == 1 && t_emb == nullptr, "EncoderUNetModel takes timesteps");
  }
  DRM_REQUIRE(ar.dry || loaded_precision[active] == precision, "precision changed after drm_unet_load_params: reload the parameters");
  Ctx c{&ar, s, N, precision};
  const float* Wb = wsets[active];
  const int mc = desc.model_channels;

  // statistics pool: sized by a dry pass (cached per shape), zeroed once
  ar.st_active = true;
  ar.st_off = 0;
  if (!ar.dry) {
    const auto key = std::make_tuple(N, H, W, precision);  // the split modes carve their split-K ticket counters out of the pool
    auto it = stats_pool_cache.find(key);
    if (it == stats_pool_cache.end()) {
      Arena probe;
      DRM_TRY(dry_forward(N, H, W, probe));
      it = stats_pool_cache.emplace(key, probe.st_off).first;
    }
    ar.st_cap = it->second;
    ar.st_base = reinterpret_cast<char*>(ar.alloc_bytes(ar.st_cap));
    if (ar.st_base) DRM_HIP_CHECK(hipMemsetAsync(ar.st_base, 0, ar.st_cap, s));
  }
  struct PoolScope {  // the pool belongs to this pass only
    Arena& a;
    ~PoolScope() {
      if (a.dry) a.peak += (a.st_off + 255) & ~size_t(255);
      a.st_active = false;
      a.st_base = nullptr;
    }
  } pool_scope{ar};

  const bool stem_direct = stem_direct_w >= 0;
  Act xin;
  const int amax_parts = pack_input_absmax_parts(H, W);
  unsigned* amax = nullptr;
  if (!stem_direct) {
    xin = new_act(c, in_cp, H, W);
    amax = c.ar->alloc<unsigned>((size_t)N * amax_parts);  // max |input| per (image, pack block): every word is written by the pack kernel
  }
  float* temb = c.ar->alloc<float>((size_t)N * mc);
  float* e1 = c.ar->alloc<float>((size_t)N * emb_dim);
  float* emb = c.ar->alloc<float>((size_t)N * emb_dim);
  float* emb_all = c.ar->alloc<float>((size_t)N * emb_total);
  DRM_TRY(arena_ok(c));
  if (!c.dry()) {
    if (!stem_direct) DRM_TRY(launch_pack_input(x, cond, rows, xin.p, N, H, W, Cx, Cc, in_cp, s, amax));
    const float* te = t_emb;
    if (!te) {
      DRM_TRY(launch_timestep_embedding(t, tf, temb, N, mc, s));
      te = temb;
    }
    DRM_TRY(launch_linear(te, Wb + te0_w, Wb + te0_b, e1, N, mc, emb_dim, 0, 1, s));
    DRM_TRY(launch_linear(e1, Wb + te2_w, Wb + te2_b, emb, N, emb_dim, emb_dim, 0, 0, s));
    DRM_TRY(launch_linear(emb, Wb + embcat_w, Wb + embcat_b, emb_all, N, emb_dim, emb_total, 1, 0, s));
  }

  std::deque<Act> acts;  // stable addresses: the skip stack and `h` share cached GroupNorm moments
  auto make = [&](int C_, int H_, int W_) -> Act* {
    acts.push_back(new_act(c, C_, H_, W_));
    return &acts.back();
  };
  std::vector<Act*> hs;
  Act* h = make(mc, H, W);
  if (stem_direct) {
    // stem conv on the NCHW boundary tensors (cat, row gather, exact fp32 products and the output's GroupNorm sums in one launch: stemhead.hip)
    DRM_TRY(expect_raw_sums(c, *h));
    if (!c.dry()) DRM_TRY(launch_stem_conv(x, Cx, cond, Cc, rows, Wb + stem_direct_w, Wb + stem_b, h->p, h->mom, N, H, W, mc, precision == PREC_FP32, s));
  } else {
    ConvArgs a;  // stem conv: raw network input
    a.C0 = in_cp; a.N = N; a.H = H; a.W = W; a.taps = 9; a.Cout = mc;
    const ConvPlan pa = plan_conv(a, precision);
    DRM_TRY(raw_input_guard(c, a, pa, nullptr, 0, 0, nullptr, amax, in_cp, amax_parts));
    if (!c.dry()) {
      a.src0 = xin.p; a.w = Wb + stem_w; a.bias = Wb + stem_b; a.out = h->p; a.cin_real = desc.in_channels;
      DRM_TRY(run_conv(c, a, pa, Wb, stem_s, h));
    }
  }
  hs.push_back(h);

  Act* pool_buf = nullptr;   // the output tensor of the Downsample that follows the block being run (allocated ahead of it) ...
  bool pool_done = false;    // ... already written, statistics included, by that block's out_layers conv
  auto run_layers = [&](std::vector<Layer>& ls, Act* skip, bool down_next = false) -> int {
    for (size_t li = 0; li < ls.size(); ++li) {
      Layer& l = ls[li];
      if (l.kind == Layer::RES) {
        Act* o = make(l.res.cout, h->H, h->W);
        Act* po = nullptr;
        bool pooled = false;
        if (down_next && li + 1 == ls.size() && h->H % 2 == 0 && h->W % 2 == 0) po = make(l.res.cout, h->H / 2, h->W / 2);
        DRM_TRY(run_resblock(c, Wb, l.res, *h, (li == 0) ? skip : nullptr, emb_all, emb_total, *o, po, &pooled));
        pool_buf = po;
        pool_done = pooled;
        h = o;
      } else if (l.kind == Layer::ATTN) {
        Act* o = make(l.attn.ch, h->H, h->W);
        DRM_TRY(run_attention(c, Wb, l.attn, *h, *o));
        h = o;
      } else if (l.kind == Layer::DOWN) {
        DRM_REQUIRE(!h->up, "downsample of an upsampled tensor");
        Act* o = pool_buf ? pool_buf : make(h->C, h->H / 2, h->W / 2);
        const bool done = pool_buf && pool_done;  // written by the producing conv's epilogue, statistics included
        pool_buf = nullptr;
        pool_done = false;
        DRM_TRY(arena_ok(c));
        if (done) {
          h = o;
          continue;
        }
        if (!c.dry()) {
          DRM_TRY(expect_raw_sums(c, *o));
          DRM_TRY(launch_avgpool2(h->p, o->p, N, h->H, h->W, h->C, s, o->mom));  // pooled tensor + its GroupNorm sums in one pass
        }
        h = o;
      } else {  // UP: nearest x2, folded into the consumer (moments are unchanged by replication)
        DRM_REQUIRE(!h->up, "double upsample");
        h->up = 1;
        h->H *= 2;
        h->W *= 2;
      }
    }
    return DRM_OK;
  };

  for (size_t b = 1; b < input_blocks.size(); ++b) {
    const bool down_next = b + 1 < input_blocks.size() && input_blocks[b + 1].size() == 1 && input_blocks[b + 1][0].kind == Layer::DOWN;
    DRM_TRY(run_layers(input_blocks[b], nullptr, down_next));
    hs.push_back(h);
  }
  DRM_TRY(run_layers(middle, nullptr));
  for (auto& blk : output_blocks) {
    Act* skip = hs.back();
    hs.pop_back();
    DRM_TRY(run_layers(blk, skip));
  }

  // head
  DRM_REQUIRE(!h->up && h->C == final_ch, "head input");
  float* sc = c.ar->alloc<float>((size_t)N * final_ch);
  float* sh = c.ar->alloc<float>((size_t)N * final_ch);
  DRM_TRY(arena_ok(c));
  DRM_TRY(gn_params(c, *h, nullptr, Wb + on_w, Wb + on_b, sc, sh, nullptr, nullptr));
  if (!c.dry()) {
    if (desc.kind == 0) {
      ConvArgs a;
      a.src0 = h->p; a.C0 = final_ch; a.N = N; a.H = h->H; a.W = h->W;
      a.gn_scale = sc; a.gn_shift = sh; a.silu = 1;
      a.w = Wb + oc_w; a.bias = Wb + oc_b; a.taps = 9; a.Cout = out_cp;
      a.out = out; a.out_nchw = 1; a.cout_valid = desc.out_channels;
      DRM_TRY(run_conv(c, a, plan_conv(a, precision), Wb, oc_s));
    } else {
      DRM_TRY(launch_encoder_head(h->p, sc, sh, Wb + oc_w, Wb + oc_b, out, N, h->H * h->W, final_ch, desc.out_channels, s));
    }
  }
  if (ar.failed) {
    set_error("workspace too small: need " + std::to_string(ar.peak) + " bytes, got " + std::to_string(ar.cap));
    return DRM_ERR_WORKSPACE;
  }
  return DRM_OK;
}

}  // namespace drm

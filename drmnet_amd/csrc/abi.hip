// extern "C" surface of libdrmnet_hip.so (declared in include/drmnet_hip.h).
#include <atomic>
#include <cstring>
#include <memory>

#include "bvh.h"
#include "profiler.h"
#include "samplers.h"

using namespace drm;

struct drm_unet {
  UNet net;
};
struct drm_drmnet {
  DrmnetSampler s;
};

namespace {

int make_arena(Arena& ar, void* ws, size_t bytes, size_t need) {
  if (need == 0) return DRM_ERR_INVALID;  // error text already set by the dry run
  if (bytes < need || ws == nullptr) {
    set_error("workspace too small: need " + std::to_string(need) + " bytes, got " + std::to_string(bytes));
    return DRM_ERR_WORKSPACE;
  }
  ar.base = static_cast<char*>(ws);
  ar.cap = bytes;
  return DRM_OK;
}

template <typename F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    set_error(std::string("exception: ") + e.what());
    return DRM_ERR_STATE;
  } catch (...) {
    set_error("unknown exception");
    return DRM_ERR_STATE;
  }
}

// shared driver for the block-level ops (tests / per-module drop-ins only): runs `body` twice (measure, then execute) over a private scratch arena
template <typename Body>
int with_scratch(hipStream_t s, Body&& body) {
  Arena dry;
  dry.dry = true;
  DRM_TRY(body(dry));
  Scratch sc(s);
  DRM_TRY(sc.reserve(dry.peak + 256));
  Arena ar;
  ar.base = static_cast<char*>(sc.p);
  ar.cap = dry.peak + 256;
  DRM_HIP_CHECK(hipMemsetAsync(sc.p, 0, ar.cap, s));
  DRM_TRY(body(ar));
  DRM_HIP_CHECK(hipStreamSynchronize(s));
  return DRM_OK;
}

// Arithmetic of the drm_op_* entry points (drm_set_op_precision).  The one piece of process-wide state behind the C ABI: an atomic word that every
// drm_op_* call reads ONCE at entry (a call runs in one mode from its weight packing to its last launch); a concurrent drm_set_op_precision takes
// effect for calls that start after it.  The network / sampler handles carry their own mode (drm_unet_set_precision).
std::atomic<int> g_op_precision{PREC_FP32};

// the weights of a block-level op: its one-layer table packed from the caller's tensors (they arrive in the table's order) by the code a network's
// load runs, into *wbuf; buffers from the call's scratch arena in both passes of with_scratch, launches in the real pass only
int pack_block(const ParamTable& tab, const float* const* params, int count, Arena& ar, int precision, hipStream_t s, float** wbuf) {
  *wbuf = ar.alloc<float>(tab.wbuf_floats);
  float* staging = ar.alloc<float>(tab.staging_floats());
  if (ar.dry) return DRM_OK;
  return tab.pack(params, count, *wbuf, precision, staging, s);
}

size_t unet_ws(UNet& net, int N, int H, int W) {
  Arena a;
  if (net.dry_forward(N, H, W, a) != DRM_OK) return 0;
  return a.peak + 256;
}

// the DDIM / DDPM chain entry points: the options (null: none) checked, the caller's workspace as the arena, then the chain over both
template <typename Body>
int run_chain(drm_unet* net, const ChainIO& io, const drm_sampler_options* opt, void* workspace, size_t workspace_bytes, Body&& chain) {
  DRM_REQUIRE(net && io.x && io.cond, "null argument");
  drm_sampler_options o{};
  if (opt) {
    DRM_REQUIRE_SIZE(opt, drm_sampler_options);
    if (opt->blend) DRM_REQUIRE_SIZE(opt->blend, drm_mask_blend);
    o = *opt;
  }
  Arena ar;
  DRM_TRY(make_arena(ar, workspace, workspace_bytes, sampler_workspace_bytes(&net->net, io.N, io.H, io.W)));
  return chain(o, ar);
}

}  // namespace

extern "C" {

int drm_abi_version(void) { return DRM_ABI_VERSION; }
const char* drm_last_error(void) { return last_error(); }

int drm_unet_create(const drm_unet_desc* desc, drm_unet** out) {
  return guarded([&]() -> int {
    DRM_REQUIRE(desc && out, "null argument");
    std::unique_ptr<drm_unet> h(new drm_unet());
    DRM_TRY(h->net.build(*desc));
    *out = h.release();
    return DRM_OK;
  });
}
void drm_unet_destroy(drm_unet* net) { delete net; }

int drm_unet_param_count(const drm_unet* net) { return net ? (int)net->net.params.size() : -1; }

int drm_unet_param_info(const drm_unet* net, int index, char* name, int name_cap, int64_t shape[4], int* ndim) {
  return guarded([&]() -> int {
    DRM_REQUIRE(net && index >= 0 && index < (int)net->net.params.size(), "param index");
    const ParamSlot& p = net->net.params[index];
    if (name && name_cap > 0) {
      std::strncpy(name, p.name.c_str(), name_cap - 1);
      name[name_cap - 1] = 0;
    }
    if (ndim) *ndim = (int)p.shape.size();
    if (shape)
      for (size_t i = 0; i < 4; ++i) shape[i] = i < p.shape.size() ? p.shape[i] : 1;
    return DRM_OK;
  });
}

int drm_unet_load_params(drm_unet* net, const float* const* ptrs, int count, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(net && ptrs, "null argument");
    return net->net.load(ptrs, count, static_cast<hipStream_t>(stream), net->net.active);
  });
}

int drm_unet_load_params_set(drm_unet* net, int set, const float* const* ptrs, int count, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(net && ptrs, "null argument");
    return net->net.load(ptrs, count, static_cast<hipStream_t>(stream), set);
  });
}

int drm_unet_use_set(drm_unet* net, int set) {
  return guarded([&]() -> int {
    DRM_REQUIRE(net && set >= 0 && set < UNet::NSETS, "weight set index");
    net->net.active = set;
    return DRM_OK;
  });
}

size_t drm_unet_workspace_bytes(const drm_unet* net, int N, int H, int W) {
  if (!net) return 0;
  size_t r = 0;
  guarded([&]() -> int {
    r = unet_ws(const_cast<drm_unet*>(net)->net, N, H, W);
    return DRM_OK;
  });
  return r;
}

int drm_unet_forward(drm_unet* net, const float* x, int Cx, const float* cond, int Cc, const int32_t* rows, const float* t_emb,
                     const int64_t* timesteps, const float* timesteps_f, float* out, int N, int H, int W, void* workspace,
                     size_t workspace_bytes, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(net && x && out, "null argument");
    DRM_REQUIRE(Cc == 0 || cond, "cond is null but Cc > 0");
    Arena ar;
    DRM_TRY(make_arena(ar, workspace, workspace_bytes, unet_ws(net->net, N, H, W)));
    return net->net.forward(x, Cx, cond, Cc, rows, t_emb, timesteps, timesteps_f, out, N, H, W, ar, static_cast<hipStream_t>(stream));
  });
}

// ------------------------------------------------------------------------------------------------ primitive ops

int drm_linear_forward(const float* in, const float* w, const float* b, float* out, int N, int I, int O, int silu_in, int silu_out, void* stream) {
  return guarded([&]() -> int { return launch_linear(in, w, b, out, N, I, O, silu_in, silu_out, static_cast<hipStream_t>(stream)); });
}

int drm_timestep_embedding(const int64_t* timesteps, float* out, int N, int dim, void* stream) {
  return guarded([&]() -> int { return launch_timestep_embedding(timesteps, nullptr, out, N, dim, static_cast<hipStream_t>(stream)); });
}

int drm_op_norm_act_conv(const float* x, const float* gamma, const float* beta, int silu, const float* w, const float* b, int ksize,
                         const float* emb, const float* residual, float* out, int N, int Cin, int Cout, int H, int W, void* stream) {
  return guarded([&]() -> int {
    hipStream_t s = static_cast<hipStream_t>(stream);
    DRM_REQUIRE(ksize == 1 || ksize == 3, "ksize");
    DRM_REQUIRE((gamma == nullptr) == (beta == nullptr), "gamma/beta");
    DRM_REQUIRE(!gamma || Cin % 32 == 0, "GroupNorm32 needs Cin % 32 == 0");
    const int taps = ksize * ksize;
    const int cinp = (ksize == 1) ? (Cin + 31) / 32 * 32 : (Cin + 7) / 8 * 8, coutp = (Cout + 31) / 32 * 32;
    DRM_REQUIRE((!residual && !emb) || Cout == coutp, "residual/emb need Cout % 32 == 0");
    const size_t hw = (size_t)H * W;
    return with_scratch(s, [&](Arena& ar) -> int {
      const int op_prec = g_op_precision.load(std::memory_order_relaxed);  // (read once: the whole call runs in this mode)
      Ctx c{&ar, s, N, op_prec};
      Act xa = new_act(c, cinp, H, W);
      float* wb = ar.alloc<float>(64);  // base for offsets: [0..63] = scale slot, then scratch
      float* scratch = ar.alloc<float>(64);
      float* wp = ar.alloc<float>(packed_conv_weight_floats(taps, coutp, cinp));
      float* bp = ar.alloc<float>(coutp);
      float* sc = ar.alloc<float>((size_t)N * cinp);
      float* sh = ar.alloc<float>((size_t)N * cinp);
      float* resn = ar.alloc<float>(N * hw * coutp);
      float* gp = ar.alloc<float>(cinp);
      float* bpn = ar.alloc<float>(cinp);
      ConvArgs a;
      a.C0 = cinp; a.N = N; a.H = H; a.W = W; a.taps = taps; a.Cout = coutp; a.out_nchw = 1; a.cout_valid = Cout;
      const ConvPlan p = plan_conv(a, op_prec);
      if (ar.dry) {
        xa.mom_valid = false;
        DRM_TRY(ensure_moments(c, xa));
        if (!gamma) DRM_TRY(raw_input_guard(c, a, p, &xa, 0, cinp, nullptr, nullptr, cinp));
        return DRM_OK;
      }
      DRM_TRY(launch_pack_input(x, nullptr, nullptr, xa.p, N, H, W, Cin, 0, cinp, s));
      DRM_TRY(pack_conv_image(op_prec, w, wp, wb, reinterpret_cast<unsigned*>(scratch), Cout, Cin, taps, coutp, cinp, false, s));
      if (b) DRM_HIP_CHECK(hipMemcpyAsync(bp, b, Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
      if (!gamma) {
        xa.mom_valid = false;
        DRM_TRY(ensure_moments(c, xa));
        DRM_TRY(raw_input_guard(c, a, p, &xa, 0, cinp, nullptr, nullptr, cinp));
      }
      if (gamma) {
        DRM_HIP_CHECK(hipMemcpyAsync(gp, gamma, Cin * sizeof(float), hipMemcpyDeviceToDevice, s));
        DRM_HIP_CHECK(hipMemcpyAsync(bpn, beta, Cin * sizeof(float), hipMemcpyDeviceToDevice, s));
        DRM_TRY(gn_params(c, xa, nullptr, gp, bpn, sc, sh));
        a.gn_scale = sc; a.gn_shift = sh;
      }
      if (residual) {
        DRM_TRY(launch_nchw_to_nhwc(residual, resn, N, H, W, Cout, s));
        a.res = resn;
      }
      a.src0 = xa.p; a.silu = silu;
      a.w = wp; a.bias = bp;
      a.emb = emb; a.emb_stride = Cout;
      a.out = out; a.cin_real = Cin;
      return run_conv(c, a, p, wb, 0);
    });
  });
}

int drm_op_resblock(const float* x0, int C0, int up0, const float* x1, int C1, const float* emb, int emb_dim, const float* const* params,
                    int n_params, float* out, int N, int Cout, int H, int W, void* stream) {
  return guarded([&]() -> int {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cin = C0 + C1;
    const bool has_skip = cin != Cout;
    DRM_REQUIRE(n_params == (has_skip ? 12 : 10), "resblock expects 10 params (12 with skip_connection)");
    DRM_REQUIRE(cin % 32 == 0 && Cout % 32 == 0 && C0 % 32 == 0, "channels % 32");
    DRM_REQUIRE(emb_dim <= 512, "emb_dim <= 512");
    return with_scratch(s, [&](Arena& ar) -> int {
      const int op_prec = g_op_precision.load(std::memory_order_relaxed);  // (read once: the whole call runs in this mode)
      Ctx c{&ar, s, N, op_prec};
      ParamTable tab;
      tab.emb_dim = emb_dim;
      Layer l;
      tab.add_res(l, "", cin, Cout, up0 ? C0 : 0);
      tab.finish();
      float* wb = nullptr;
      DRM_TRY(pack_block(tab, params, n_params, ar, op_prec, s, &wb));
      float* e_out = ar.alloc<float>((size_t)N * Cout);
      Act a0 = new_act(c, C0, H, W);
      a0.up = up0;
      Act a1 = new_act(c, C1 > 0 ? C1 : 4, H, W);
      Act o = new_act(c, Cout, H, W);
      if (!ar.dry) {
        DRM_TRY(launch_linear(emb, wb + tab.embcat_w, wb + tab.embcat_b, e_out, N, emb_dim, tab.emb_total, 1, 0, s));
        DRM_TRY(launch_nchw_to_nhwc(x0, a0.p, N, H >> up0, W >> up0, C0, s));
        if (C1 > 0) DRM_TRY(launch_nchw_to_nhwc(x1, a1.p, N, H, W, C1, s));
      }
      DRM_TRY(run_resblock(c, wb, l.res, a0, C1 > 0 ? &a1 : nullptr, e_out, tab.emb_total, o));
      if (!ar.dry) DRM_TRY(launch_nhwc_to_nchw(o.p, out, N, H, W, Cout, s));
      return DRM_OK;
    });
  });
}

int drm_op_attention_block(const float* x, const float* const* params, float* out, int N, int C, int H, int W, void* stream) {
  return guarded([&]() -> int {
    hipStream_t s = static_cast<hipStream_t>(stream);
    DRM_REQUIRE(C % 32 == 0, "channels % 32");
    return with_scratch(s, [&](Arena& ar) -> int {
      const int op_prec = g_op_precision.load(std::memory_order_relaxed);  // (read once: the whole call runs in this mode)
      Ctx c{&ar, s, N, op_prec};
      ParamTable tab;
      Layer l;
      tab.add_attn(l, "", C);
      tab.finish();
      float* wb = nullptr;
      DRM_TRY(pack_block(tab, params, 6, ar, op_prec, s, &wb));
      Act a = new_act(c, C, H, W);
      Act o = new_act(c, C, H, W);
      if (!ar.dry) DRM_TRY(launch_nchw_to_nhwc(x, a.p, N, H, W, C, s));
      DRM_TRY(run_attention(c, wb, l.attn, a, o));
      if (!ar.dry) DRM_TRY(launch_nhwc_to_nchw(o.p, out, N, H, W, C, s));
      return DRM_OK;
    });
  });
}

int drm_op_stem_conv(const float* x, int Cx, const float* cond, int Cc, const int32_t* rows, const float* w, const float* b, float* out, double* stat,
                     int N, int Cout, int H, int W, void* stream) {
  return guarded([&]() -> int {
    hipStream_t s = static_cast<hipStream_t>(stream);
    DRM_REQUIRE(x && w && out, "stem conv: x, w and out must not be null");
    DRM_REQUIRE(Cx >= 1 && Cc >= 0 && (Cc == 0 || cond), "stem conv: cond is null but Cc > 0");
    DRM_REQUIRE(stem_direct_applicable(Cx + Cc, Cout), "stem conv: Cx + Cc must be 4 or 6 and Cout must be 128 (got Cx + Cc = " + std::to_string(Cx + Cc) +
                                                           ", Cout = " + std::to_string(Cout) + ")");
    DRM_REQUIRE(N >= 1 && H >= 1 && W >= 1, "stem conv: N, H, W");
    return with_scratch(s, [&](Arena& ar) -> int {
      const bool exact = g_op_precision.load(std::memory_order_relaxed) == PREC_FP32;  // (read once: the whole call runs in this form)
      float* wimg = ar.alloc<float>(stem_weight_floats());
      float* bz = ar.alloc<float>(Cout);  // (the scratch is zeroed: the bias of a call without one)
      float* nhwc = ar.alloc<float>((size_t)N * H * W * Cout);
      if (ar.dry) return DRM_OK;
      if (stat) DRM_HIP_CHECK(hipMemsetAsync(stat, 0, (size_t)N * Cout * sizeof(double2), s));
      DRM_TRY(launch_pack_stem_weight(w, wimg, Cout, Cx + Cc, exact, s));
      DRM_TRY(launch_stem_conv(x, Cx, cond, Cc, rows, wimg, b ? b : bz, nhwc, reinterpret_cast<double2*>(stat), N, H, W, Cout, exact, s));
      return launch_nhwc_to_nchw(nhwc, out, N, H, W, Cout, s);
    });
  });
}

int drm_op_avgpool2(const float* x, float* out, double* stat, int N, int C, int H, int W, void* stream) {
  return guarded([&]() -> int {
    hipStream_t s = static_cast<hipStream_t>(stream);
    DRM_REQUIRE(x && out, "avgpool2: x and out must not be null");
    DRM_REQUIRE(C >= 4 && C % 4 == 0, "avgpool2: C must be a multiple of 4 (got C = " + std::to_string(C) + ")");
    DRM_REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "avgpool2: H and W must be even (got H = " + std::to_string(H) + ", W = " + std::to_string(W) + ")");
    DRM_REQUIRE(N >= 1, "avgpool2: N");
    return with_scratch(s, [&](Arena& ar) -> int {
      float* xin = ar.alloc<float>((size_t)N * H * W * C);
      float* pooled = ar.alloc<float>((size_t)N * (H / 2) * (W / 2) * C);
      if (ar.dry) return DRM_OK;
      if (stat) DRM_HIP_CHECK(hipMemsetAsync(stat, 0, (size_t)N * C * sizeof(double2), s));
      DRM_TRY(launch_nchw_to_nhwc(x, xin, N, H, W, C, s));
      DRM_TRY(launch_avgpool2(xin, pooled, N, H, W, C, s, reinterpret_cast<double2*>(stat)));
      return launch_nhwc_to_nchw(pooled, out, N, H / 2, W / 2, C, s);
    });
  });
}

int drm_op_encoder_head(const float* x, const float* scale, const float* shift, const float* w, const float* b, float* out, int N, int C, int H, int W,
                        int O, void* stream) {
  return guarded([&]() -> int {
    hipStream_t s = static_cast<hipStream_t>(stream);
    DRM_REQUIRE(x && scale && shift && w && b && out, "encoder head: null argument");
    DRM_REQUIRE(C >= 4 && C % 4 == 0, "encoder head: C must be a multiple of 4 (got C = " + std::to_string(C) + ")");
    DRM_REQUIRE(N >= 1 && H >= 1 && W >= 1 && O >= 1, "encoder head: N, H, W, O");
    return with_scratch(s, [&](Arena& ar) -> int {
      float* xin = ar.alloc<float>((size_t)N * H * W * C);
      if (ar.dry) return DRM_OK;
      DRM_TRY(launch_nchw_to_nhwc(x, xin, N, H, W, C, s));
      return launch_encoder_head(xin, scale, shift, w, b, out, N, H * W, C, O, s);
    });
  });
}

// ------------------------------------------------------------------------------------------------ samplers

int drm_drmnet_create(drm_unet* illnet, drm_unet* refnet, const float* const* zemb, const drm_drmnet_cfg* cfg, drm_drmnet** out) {
  return guarded([&]() -> int {
    DRM_REQUIRE(illnet && refnet && zemb && cfg && out, "null argument");
    std::unique_ptr<drm_drmnet> h(new drm_drmnet());
    DRM_TRY(h->s.init(&illnet->net, &refnet->net, zemb, *cfg));
    *out = h.release();
    return DRM_OK;
  });
}
void drm_drmnet_destroy(drm_drmnet* s) { delete s; }

size_t drm_drmnet_workspace_bytes(const drm_drmnet* s, int N, int H, int W) {
  if (!s) return 0;
  size_t r = 0;
  guarded([&]() -> int {
    r = s->s.workspace_bytes(N, H, W);
    return DRM_OK;
  });
  return r;
}

int drm_drmnet_set_batch_parts(drm_drmnet* s, int parts) {
  return guarded([&]() -> int {
    DRM_REQUIRE(s != nullptr, "drm_drmnet_set_batch_parts: null handle");
    DRM_REQUIRE(parts >= 1 && parts <= DrmnetSampler::PART_MAX, "drm_drmnet_set_batch_parts: 1 .. 4 parts");
    s->s.parts = parts;
    return DRM_OK;
  });
}

int drm_drmnet_set_batch_part_min(drm_drmnet* s, int rows) {
  return guarded([&]() -> int {
    DRM_REQUIRE(s != nullptr, "drm_drmnet_set_batch_part_min: null handle");
    DRM_REQUIRE(rows >= 1, "drm_drmnet_set_batch_part_min: at least one row per part");
    s->s.part_min = rows;
    return DRM_OK;
  });
}

int drm_drmnet_step(drm_drmnet* s, float* Lr_k, const float* LrK, const int32_t* rows, int n_active, int step, const float* noise,
                    uint64_t seed, float* zk_out, float* zK_out, int32_t* converged_out, int B, int H, int W, void* workspace,
                    size_t workspace_bytes, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(s && Lr_k && LrK, "null argument");
    Arena ar;
    DRM_TRY(make_arena(ar, workspace, workspace_bytes, s->s.workspace_bytes(n_active, H, W)));
    return s->s.step(Lr_k, LrK, rows, n_active, step, noise, seed, zk_out, zK_out, converged_out, B, H, W, ar, static_cast<hipStream_t>(stream));
  });
}

int drm_drmnet_sample(drm_drmnet* s, const float* LrK, const float* cond, const float* noise0, const float* step_noise, uint64_t seed, int early_exit,
                      float* Lr0, float* zK, int32_t* K, int32_t* steps_done, int B, int H, int W, void* workspace, size_t workspace_bytes,
                      void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(s && LrK && cond && Lr0 && zK && K, "null argument");
    Arena ar;
    DRM_TRY(make_arena(ar, workspace, workspace_bytes, s->s.workspace_bytes(B, H, W)));
    return s->s.sample(LrK, cond, noise0, step_noise, seed, early_exit, Lr0, zK, K, steps_done, B, H, W, ar, static_cast<hipStream_t>(stream));
  });
}

size_t drm_sampler_workspace_bytes(const drm_unet* net, int N, int H, int W) {
  if (!net) return 0;
  size_t r = 0;
  guarded([&]() -> int {
    r = sampler_workspace_bytes(&const_cast<drm_unet*>(net)->net, N, H, W);
    return DRM_OK;
  });
  return r;
}

int drm_ddim_sample(drm_unet* net, float* x, const float* cond, const int64_t* timesteps, const float* coef, int S, int num_steps,
                    const float* noise, uint64_t seed, const drm_sampler_options* opt, const drm_chain_log* log, int N, int H, int W,
                    void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&]() -> int {
    drm_chain_log lg{};
    if (log) {
      DRM_REQUIRE_SIZE(log, drm_chain_log);
      DRM_REQUIRE(log->every_t <= 0 || (log->x && log->pred_x0 && log->slots > 0), "ddim intermediates: both log buffers and their slot count");
      lg = *log;
      if (lg.every_t <= 0) lg.every_t = 0, lg.x = lg.pred_x0 = nullptr;  // (no intermediates, whatever the buffers)
    }
    const ChainIO io{x, cond, noise, seed, N, H, W};
    return run_chain(net, io, opt, workspace, workspace_bytes, [&](const drm_sampler_options& o, Arena& ar) {
      return ddim_sample(&net->net, io, timesteps, coef, S, num_steps, lg, o, ar, static_cast<hipStream_t>(stream));
    });
  });
}

int drm_ddpm_sample(drm_unet* net, float* x, float* pred_x0, const float* cond, const float* coef, int T_start, int clip_denoised,
                    const float* noise, uint64_t seed, const drm_sampler_options* opt, int N, int H, int W, void* workspace, size_t workspace_bytes,
                    void* stream) {
  return guarded([&]() -> int {
    const ChainIO io{x, cond, noise, seed, N, H, W};
    return run_chain(net, io, opt, workspace, workspace_bytes, [&](const drm_sampler_options& o, Arena& ar) {
      DRM_REQUIRE(o.uncond == nullptr, "drm_ddpm_sample: classifier-free guidance exists on the DDIM chain only (ddim.py:225-232; ddpm.py p_sample has none)");
      return ddpm_sample(&net->net, io, pred_x0, coef, T_start, clip_denoised, o, ar, static_cast<hipStream_t>(stream));
    });
  });
}

int drm_unet_set_precision(drm_unet* net, int precision) {
  return guarded([&]() -> int {
    DRM_REQUIRE(net && precision_valid(precision),
                "precision must be 0 (fp32 MFMA), 1 (split fp16 x3), 2 (plain fp16 operands), 3 (split fp16 with fp8 cross terms) or 4 (plain bf16 operands)");
    net->net.precision = precision;
    return DRM_OK;
  });
}
int drm_set_op_precision(int precision) {
  return guarded([&]() -> int {
    DRM_REQUIRE(precision_valid(precision),
                "precision must be 0 (fp32 MFMA), 1 (split fp16 x3), 2 (plain fp16 operands), 3 (split fp16 with fp8 cross terms) or 4 (plain bf16 operands)");
    g_op_precision.store(precision, std::memory_order_relaxed);
    return DRM_OK;
  });
}

int drm_set_upconv_split(int mode) {
  return guarded([&]() -> int {
    DRM_REQUIRE(mode >= 0 && mode <= 2, "upconv split mode: 0 = never, 1 = by the measured rule, 2 = wherever the form applies");
    set_upconv_split(mode);
    return DRM_OK;
  });
}

int drm_set_graph_replay(int on) {
  set_graph_replay(on != 0);
  return DRM_OK;
}
int64_t drm_graph_launches(void) { return (int64_t)graph_launches(); }

void drm_profile_enable(int on) { prof_enable(on); }
void drm_profile_reset(void) { prof_reset(); }
int drm_profile_collect(double* ms, double* flops, double* bytes, int64_t* launches) {
  return guarded([&]() -> int {
    DRM_REQUIRE(ms && flops && bytes && launches, "null argument");
    prof_collect(ms, flops, bytes, launches);
    return DRM_OK;
  });
}

int drm_randn(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream) {
  return guarded([&]() -> int { return launch_randn(out, n, seed, offset, static_cast<hipStream_t>(stream)); });
}

size_t drm_refmap_workspace_bytes(int64_t n, int res, float angle_threshold) {
  if (n < 0 || res <= 0 || !(angle_threshold >= 0.f)) return 0;
  return refmap_workspace_bytes(n, res, angle_threshold);
}

int drm_refmap_mask_make(const float* colors, const float* normals, int64_t n, int channels, int res, float angle_threshold, int min_points,
                         float* refmap, uint8_t* refmask, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(refmap && refmask && workspace && (n == 0 || (colors && normals)), "drm_refmap_mask_make: null pointer");
    return launch_refmap_mask_make(colors, normals, n, channels, res, angle_threshold, min_points, refmap, refmask, workspace, workspace_bytes,
                                   static_cast<hipStream_t>(stream));
  });
}

int drm_erode_mask(const uint8_t* mask, int H, int W, int kernel_size, uint8_t* out, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(mask && out, "drm_erode_mask: null pointer");
    return launch_erode_mask(mask, H, W, kernel_size, out, static_cast<hipStream_t>(stream));
  });
}

// ------------------------------------------------------------------------------------------------ boundary maps (transform.hip)

int drm_map_chain(const float* x, float* out, int64_t per_image, int B, const int32_t* ops, const float* args, int n_ops, const float* lo,
                  const float* hi, const float* scale, void* stream) {
  return guarded([&]() -> int { return launch_map_chain(x, out, per_image, B, ops, args, n_ops, lo, hi, scale, static_cast<hipStream_t>(stream)); });
}

int drm_masked_log_range(const float* x, const float* mask, int B, int C, int HW, float* lo, float* hi, void* stream) {
  return guarded([&]() -> int { return launch_masked_log_range(x, mask, B, C, HW, lo, hi, static_cast<hipStream_t>(stream)); });
}

int drm_luminance_scale(const float* x, int B, int HW, float scaler, float* scale, void* stream) {
  return guarded([&]() -> int { return launch_luminance_scale(x, B, HW, scaler, scale, static_cast<hipStream_t>(stream)); });
}

int drm_mirmap2envmap(const float* mirmap, const float* basis, float* out, int B, int C, int H, int W, int OH, int OW, int log_scale_interpolation,
                      int channels_last, void* stream) {
  return guarded([&]() -> int {
    return launch_mirmap2envmap(mirmap, basis, out, B, C, H, W, OH, OW, log_scale_interpolation, channels_last, static_cast<hipStream_t>(stream));
  });
}

int drm_hdr2ldr(const float* x, const uint8_t* mask, int HW, float alpha, float gamma, float* out, void* stream) {
  return guarded([&]() -> int { return launch_hdr2ldr(x, mask, HW, alpha, gamma, out, static_cast<hipStream_t>(stream)); });
}

size_t drm_profile_variants(char* buf, size_t cap) { return prof_variants_text(buf, cap); }

int drm_resize(const float* x, float* out, int planes, int IH, int IW, int OH, int OW, int mode, void* stream) {
  return guarded([&]() -> int { return launch_resize(x, out, planes, IH, IW, OH, OW, mode, static_cast<hipStream_t>(stream)); });
}

// ------------------------------------------------------------------------------------------------ sphere / envmap warps (sphere_warp.hip)

int drm_envmap2mirmap(const float* envmap, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int mitigate_aliasing,
                      int log_scale_interpolation, int channels_last_in, void* stream) {
  return guarded([&]() -> int {
    return launch_envmap2mirmap(envmap, frames, out, B, C, H, W, OH, OW, mitigate_aliasing, log_scale_interpolation, channels_last_in,
                                static_cast<hipStream_t>(stream));
  });
}

int drm_rotate_envmap(const float* envmap, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int channels_last_in,
                      void* stream) {
  return guarded([&]() -> int { return launch_rotate_envmap(envmap, frames, out, B, C, H, W, OH, OW, channels_last_in, static_cast<hipStream_t>(stream)); });
}

int drm_mirimg2envmap(const float* refimg, const float* frames, float* out, int B, int C, int H, int W, int OH, int OW, int log_scale_interpolation,
                      int channels_last_in, void* stream) {
  return guarded([&]() -> int {
    return launch_mirimg2envmap(refimg, frames, out, B, C, H, W, OH, OW, log_scale_interpolation, channels_last_in, static_cast<hipStream_t>(stream));
  });
}

int drm_refmap2refimg(const float* refmap, float* out, uint8_t* mask, int B, int C, int H, int W, int radius, int channels_last_in, void* stream) {
  return guarded([&]() -> int { return launch_refmap2refimg(refmap, out, mask, B, C, H, W, radius, channels_last_in, static_cast<hipStream_t>(stream)); });
}

// ------------------------------------------------------------------------------------------------ forward model (render.hip)

int drm_render_refmap(const drm_shading* shading, int L, int R, int subpixel, int flip, float* out, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(shading, "drm_render_refmap: shading is null");
    return launch_render_refmap(*shading, L, R, subpixel, flip, out, static_cast<hipStream_t>(stream));
  });
}

size_t drm_render_light_workspace_bytes(int B, int EH, int EW, int light_samples) { return render_light_workspace_bytes(B, EH, EW, light_samples); }

size_t drm_render_mesh_workspace_bytes(int64_t F, int B, int H, int W, int subpixel) {
  return render_mesh_workspace_bytes((long long)F, B, H, W, subpixel);
}

int drm_render_mesh(const drm_shading* shading, const drm_mesh_render* mesh, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(shading && mesh, "drm_render_mesh: shading or mesh is null");
    return launch_render_mesh(*shading, *mesh, static_cast<hipStream_t>(stream));
  });
}

int drm_render_mesh_tables(const drm_shading* shading, const drm_mesh_render* mesh, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(shading && mesh, "drm_render_mesh_tables: shading or mesh is null");
    return launch_render_mesh_tables(*shading, *mesh, static_cast<hipStream_t>(stream));
  });
}

size_t drm_mesh_bvh_bytes(int64_t F) { return mesh_bvh_bytes((long long)F); }

int drm_mesh_bvh_build(const float* vertex_positions, const int32_t* faces, int64_t V, int64_t F, void* bvh, size_t bytes) {
  return guarded([&]() -> int { return mesh_bvh_build(vertex_positions, faces, (long long)V, (long long)F, bvh, bytes); });
}

int drm_mesh_occluded(const float* vertex_positions, const int32_t* faces, int64_t V, int64_t F, const void* bvh, const float* origins, const float* dirs,
                      const int32_t* exclude, int32_t* out, int64_t N, void* stream) {
  return guarded([&]() -> int {
    return launch_mesh_occluded(vertex_positions, faces, (long long)V, (long long)F, bvh, origins, dirs, exclude, out, (long long)N,
                                static_cast<hipStream_t>(stream));
  });
}

int drm_mesh_closest_hit(const float* vertex_positions, const int32_t* faces, int64_t V, int64_t F, const void* bvh, const float* origins,
                         const float* dirs, const int32_t* exclude, int32_t* out_face, float* out_tuv, int64_t N, void* stream) {
  return guarded([&]() -> int {
    return launch_mesh_closest_hit(vertex_positions, faces, (long long)V, (long long)F, bvh, origins, dirs, exclude, out_face, out_tuv, (long long)N,
                                   static_cast<hipStream_t>(stream));
  });
}

int drm_render_normals(const drm_shading* shading, const float* normals, const uint8_t* mask, int Bn, int H, int W, float* image, float* alpha,
                       void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(shading, "drm_render_normals: shading is null");
    return launch_render_normals(*shading, normals, mask, Bn, H, W, image, alpha, static_cast<hipStream_t>(stream));
  });
}

int drm_image_from_refmap(const float* refmap, const uint8_t* refmask, int Br, int R, const float* normals, const uint8_t* mask, int Bn, float* image,
                          float* alpha, int B, int H, int W, void* stream) {
  return guarded([&]() -> int {
    return launch_image_from_refmap(refmap, refmask, Br, R, normals, mask, Bn, image, alpha, B, H, W, static_cast<hipStream_t>(stream));
  });
}

int drm_brdf_eval(const float* z, int z_rows, const float* n, const float* v, const float* l, float* out, int64_t N, void* stream) {
  return guarded([&]() -> int { return launch_brdf_eval(z, z_rows, n, v, l, out, (long long)N, static_cast<hipStream_t>(stream)); });
}

// ------------------------------------------------------------------------------------------------ measured BRDFs (brdf_table.hip)

int drm_brdf_to_merl(const float* z, int rows, float* tables_out, void* stream) {
  return guarded([&]() -> int { return launch_brdf_to_merl(z, rows, tables_out, static_cast<hipStream_t>(stream)); });
}

int drm_merl_eval(const float* tables, int NT, const int32_t* table_of, const float* n, const float* v, const float* l, float* out, int64_t N, int linear,
                  void* stream) {
  return guarded([&]() -> int { return launch_merl_eval(tables, NT, table_of, n, v, l, out, (long long)N, linear, static_cast<hipStream_t>(stream)); });
}

int drm_brdf_error_sums(const float* z, int C, const float* table, const float* z_target, double* workspace, size_t workspace_bytes, double* sums,
                        void* stream) {
  return guarded([&]() -> int {
    return launch_brdf_error_sums(z, C, table, z_target, workspace, workspace_bytes, sums, static_cast<hipStream_t>(stream));
  });
}

// ------------------------------------------------------------------------------------------------ image-space errors (image_error.hip)

int drm_image_error_sums(const drm_image_error* args, void* stream) {
  return guarded([&]() -> int {
    DRM_REQUIRE(args, "drm_image_error_sums: args is null");
    return launch_image_error_sums(*args, static_cast<hipStream_t>(stream));
  });
}

// ------------------------------------------------------------------------------------------------ validation losses (losses.hip)

int drm_validation_losses(const float* model_out, const float* Lr_k, const float* Lr_km1, const int32_t* K, const float* z_out, const float* z_k,
                          const float* z_K, const int32_t* reversed_k, const float* z0, double gamma, int loss_type, double l_refmap_weight,
                          double l_refcode_weight, int B, int64_t per_row, int P, void* workspace, size_t workspace_bytes, float* out, void* stream) {
  return guarded([&]() -> int {
    return launch_validation_losses(model_out, Lr_k, Lr_km1, K, z_out, z_k, z_K, reversed_k, z0, gamma, loss_type, l_refmap_weight, l_refcode_weight, B,
                                    (long long)per_row, P, static_cast<double*>(workspace), workspace_bytes, out, static_cast<hipStream_t>(stream));
  });
}

// ------------------------------------------------------------------------------------------------ ObsNet forward process and losses (obs_forward.hip)

int drm_obs_forward_process(const float* x, const float* mask, const int32_t* t, const float* sqrt_alphas_cumprod,
                            const float* sqrt_one_minus_alphas_cumprod, int T, float noisy_observe, int padding_mode, const float* e_observe,
                            const float* e_padding, const float* e_q, uint64_t seed, float* cond, float* x_noisy, float* noise, int B, int C, int H,
                            int W, int mask_H, int mask_W, void* stream) {
  return guarded([&]() -> int {
    return launch_obs_forward_process(x, mask, t, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, T, noisy_observe, padding_mode, e_observe, e_padding,
                                      e_q, seed, cond, x_noisy, noise, B, C, H, W, mask_H, mask_W, static_cast<hipStream_t>(stream));
  });
}

int drm_diffusion_losses(const float* model_out, const float* target, const float* invmask, const int32_t* t, const float* logvar,
                         const float* lvlb_weights, int T, int loss_type, double l_simple_weight, double original_elbo_weight, int B,
                         int64_t per_row, int C, void* workspace, size_t workspace_bytes, float* out, float* loss_simple_rows, void* stream) {
  return guarded([&]() -> int {
    return launch_diffusion_losses(model_out, target, invmask, t, logvar, lvlb_weights, T, loss_type, l_simple_weight, original_elbo_weight, B,
                                   (long long)per_row, C, static_cast<double*>(workspace), workspace_bytes, out, loss_simple_rows,
                                   static_cast<hipStream_t>(stream));
  });
}

}  // extern "C"

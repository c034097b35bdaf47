// Stand-alone host check of the conv planner against the stated forms: plans every conv of a sweep of shapes with the library's own plan_conv
// (csrc/conv_plan.hip, included whole) and asserts that every pipeline plan names an instantiation that exists -- s2_form (csrc/conv_forms.h), in a
// unit of DRM_S2_UNITS -- and keeps the contracts launch_s2 (csrc/conv_split2.hip) requires of it.  Prints the case counts and a 64-bit digest
// (FNV-1a, a field per step) over every field of every plan in enumeration order: equal digests = the same plans.  Host code only, no HIP call, no GPU:
//
//   hipcc -O2 -std=c++17 --offload-host-only tools/conv_plan_check.hip -o conv_plan_check && ./conv_plan_check [--units]
//
// (for the sanitizers add -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined).  --units prints the unit numbers
// (10 * TAPS + TERMS) of DRM_S2_UNITS, one per line, and nothing else.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../drmnet_amd/csrc/conv_plan.hip"

namespace drm {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
const char* last_error() { return g_error.c_str(); }
}  // namespace drm

namespace {

using namespace drm;

bool unit_listed(int taps, int terms) {
#define DRM_X(TAPS, TERMS) if (taps == TAPS && terms == TERMS) return true;
  DRM_S2_UNITS(DRM_X)
#undef DRM_X
  return false;
}

uint64_t g_digest = 0xcbf29ce484222325ull;
void mix(uint64_t v) { g_digest = (g_digest ^ v) * 0x100000001b3ull; }

long long g_cases = 0, g_pipeline = 0, g_igemm = 0, g_none = 0, g_four_tap_skipped = 0, g_checked = 0, g_bad = 0;

void fail(const char* what, const ConvArgs& a, int precision, bool want_pool, const ConvPlan& p) {
  if (++g_bad <= 20)
    std::printf("VIOLATION %s: precision %d mx %d taps %d N %d %dx%d C %d->%d nchw %d w_img %d want_pool %d: tile %d on %dx%d terms %d ragged %d ksplit %d finish %d pool %d\n",
                what, precision, a.mx_site, a.taps, a.N, a.H, a.W, a.C0, a.Cout, a.out_nchw, (int)(a.w_img_stride_f4 != 0), (int)want_pool, (int)p.tile,
                p.th, p.tw, p.terms, (int)p.ragged, p.ksplit, (int)p.finish, (int)p.pool);
}

void check(const ConvArgs& a, int precision, bool want_pool) {
  const ConvPlan p = plan_conv(a, precision, want_pool, false);
  ++g_cases;
  for (uint64_t v : {(uint64_t)p.kernel, (uint64_t)p.terms, (uint64_t)p.tile, (uint64_t)p.th, (uint64_t)p.tw, (uint64_t)p.ragged, (uint64_t)p.kc, (uint64_t)p.ksplit,
                     (uint64_t)p.finish, (uint64_t)p.tickets, (uint64_t)p.pool, (uint64_t)p.gn_fold})
    mix(v);
  if (p.kernel != CONV_PIPELINE) {
    ++(p.kernel == CONV_IGEMM ? g_igemm : g_none);
    return;
  }
  ++g_pipeline;
  // 4-tap plans: the engine launches only the ones its plain() admits (engine.hip plan_upconv_split)
  if (a.taps == 4 && (p.ragged || p.ksplit != 1 || p.gn_fold || p.pool)) {
    ++g_four_tap_skipped;
    return;
  }
  ++g_checked;
  auto need = [&](bool ok, const char* what) {
    if (!ok) fail(what, a, precision, want_pool, p);
  };
  const bool sk = p.finish == SPLIT_IN_LAUNCH;
  const TileShape t = tile_shape(p.tile);
  need(unit_listed(a.taps, p.terms), "no unit of DRM_S2_UNITS");
  need(s2_form(a.taps, p.terms, p.th, p.tw, p.tile, p.ragged, sk, p.pool).exists, "no instantiation (s2_form)");
  need(p.ragged || (a.H % p.th == 0 && a.W % p.tw == 0), "tile does not divide the map");
  need(a.Cout % t.bn() == 0 && t.bm() % (p.th * p.tw) == 0, "GEMM tile does not divide Cout or hold whole pixel tiles");
  need(!p.pool || (p.tile == TILE_256x128 && a.taps == 9 && p.th == 16 && p.tw == 16 && p.ksplit == 1 && !a.out_nchw), "pooled form");
  need(!sk || p.tile == TILE_128x32, "in-launch split-K finish off the 128x32 tile");
  need((p.ksplit > 1) == (p.finish != SPLIT_NONE), "split factor and finish disagree");
  need(p.ksplit == 1 || (!a.out_nchw && a.w_img_stride_f4 == 0 && p.ksplit <= 8 && (a.C0 + a.C1) / 32 / p.ksplit >= 1), "split-K launch contract");
  need(a.w_img_stride_f4 == 0 || (t.bm() == p.th * p.tw && p.ksplit == 1), "per-image weights need one image per tile, un-split");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--units") == 0) {
#define DRM_X(TAPS, TERMS) std::printf("%d\n", 10 * TAPS + TERMS);
    DRM_S2_UNITS(DRM_X)
#undef DRM_X
    return 0;
  }
  const int Ns[] = {1, 2, 3, 4, 5, 8, 16, 32, 33, 64};
  const int HWs[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 20, 24, 31, 32, 33, 48, 64, 96, 128, 256};
  const int Cs[] = {32, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536};
  for (int precision = PREC_FP32; precision <= PREC_BF16; ++precision)
    for (int taps : {9, 1, 4})
      for (int mx = 0; mx <= (precision == PREC_F16MX && taps != 1 ? 1 : 0); ++mx)
        // (the 4-tap form is planned by the engine alone: NHWC, shared weights, no pool)
        for (int nchw = 0; nchw <= (taps == 4 ? 0 : 1); ++nchw)
          for (int w_img = 0; w_img <= (taps == 1 ? 1 : 0); ++w_img)
            for (int want_pool = 0; want_pool <= (taps == 4 ? 0 : 1); ++want_pool)
              for (int N : Ns)
                for (int H : HWs)
                  for (int W : HWs)
                    for (int Cin : Cs)
                      for (int Cout : Cs) {
                        ConvArgs a;
                        a.N = N; a.H = H; a.W = W; a.C0 = Cin; a.Cout = Cout; a.taps = taps;
                        a.mx_site = mx; a.out_nchw = nchw; a.w_img_stride_f4 = w_img;
                        check(a, precision, want_pool != 0);
                      }
  std::printf("%lld cases: %lld pipeline plans, %lld conv_igemm plans, %lld without a kernel\n", g_cases, g_pipeline, g_igemm, g_none);
  std::printf("%lld pipeline plans checked (%lld 4-tap plans the engine does not launch left out), %lld violations\n", g_checked, g_four_tap_skipped, g_bad);
  std::printf("digest %016llx\n", (unsigned long long)g_digest);
  return g_bad == 0 ? 0 : 1;
}

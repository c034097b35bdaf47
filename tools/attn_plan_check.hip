// Stand-alone host check of the attention planner: plans every attention core of a sweep of shapes with the library's own plan_attention
// (csrc/attn_plan.hip over csrc/conv_plan.hip, both included whole) and asserts what launch_attention_core (csrc/attn.hip) relies on: the workspace
// size is the walk of attention_tables and its carve stays inside it, the score buffer is one image group (none for the single-kernel form), the
// plans of a short last group exist exactly where the group loop reads them, the conv-pipeline form only occurs where both GEMMs are pipeline plans
// with one image per pixel tile, and the split short-sequence kernels only where their chunking holds.  Prints the case counts per form and a 64-bit
// digest (FNV-1a) over every plan in enumeration order.  Host code only, no HIP call, no GPU:
//
//   hipcc -O2 -std=c++17 --offload-host-only tools/attn_plan_check.hip -o attn_plan_check && ./attn_plan_check
//   ./attn_plan_check --case N H W C precision     (fp32 | f16x3 | f16 | f16mx | bf16): one plan, one line
//
// (for the sanitizers add -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../drmnet_amd/csrc/conv_plan.hip"
#include "../drmnet_amd/csrc/attn_plan.hip"

namespace drm {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
const char* last_error() { return g_error.c_str(); }
}  // namespace drm

namespace {

using namespace drm;

const char* const PRECISIONS[] = {"fp32", "f16x3", "f16", "f16mx", "bf16"};  // (the order of enum Precision)
const char* const FORMS[] = {"small", "conv", "flash"};

uint64_t g_digest = 0xcbf29ce484222325ull;
void mix(uint64_t v) { g_digest = (g_digest ^ v) * 0x100000001b3ull; }

long long g_cases = 0, g_form[3] = {0, 0, 0}, g_tail = 0, g_carved = 0, g_bad = 0;
std::vector<float> g_ws(1 << 20);  // plans whose workspace fits are carved for real: every table inside it, in order, none overlapping

bool one_image_pipeline(const ConvPlan& c, int T) {
  return c.kernel == CONV_PIPELINE && !c.ragged && c.ksplit == 1 && tile_shape(c.tile).bm() == c.th * c.tw && T % (c.th * c.tw) == 0;
}

void check(int N, int H, int W, int C, int precision) {
  const AttnPlan p = plan_attention(N, H, W, C, precision);
  const size_t T = (size_t)H * W;
  ++g_cases;
  ++g_form[p.form];
  for (uint64_t v : {(uint64_t)p.form, (uint64_t)p.terms, (uint64_t)p.split_qk, (uint64_t)p.split_pv, (uint64_t)p.guard, (uint64_t)p.group, (uint64_t)p.scores_floats,
                     (uint64_t)p.ws_floats, (uint64_t)p.out_stats, (uint64_t)p.qk[0].tile, (uint64_t)p.pv[0].tile, (uint64_t)p.qk[1].tile, (uint64_t)p.pv[1].tile})
    mix(v);
  auto need = [&](bool ok, const char* what) {
    if (!ok && ++g_bad <= 20)
      std::printf("VIOLATION %s: %s N %d %dx%d C %d: form %s terms %d group %d split_qk %d split_pv %d guard %d scores %zu ws %zu\n", what, PRECISIONS[precision], N,
                  H, W, C, FORMS[p.form], p.terms, p.group, (int)p.split_qk, (int)p.split_pv, (int)p.guard, p.scores_floats, p.ws_floats);
  };
  const bool flash = p.form == ATTN_FLASH, conv = p.form == ATTN_CONV, small = p.form == ATTN_SMALL;
  need(p.N == N && p.H == H && p.W == W && p.C == C && p.terms == precision_terms(precision), "plan does not restate its shape");
  need(p.group >= 1 && p.group <= N && (size_t)p.group * T * T * sizeof(float) <= std::max<size_t>((size_t)DRM_ATTN_GROUP_MIB << 20, T * T * sizeof(float)),
       "image group");
  // the workspace: the walk itself, and its size restated from the form
  size_t end = ~(size_t)0;
  attention_tables(p, nullptr, &end);
  need(end == p.ws_floats, "ws_floats is not the walk of attention_tables");
  const size_t Z = std::max<size_t>((size_t)C, T), n = (size_t)N;
  const size_t tables = n * C + n * T + n * Z + 6 * n + (conv ? 0 : n) + 64;
  const size_t want = flash ? 3 * n * T * C + tables : (conv ? 2 * n * T * C + tables : (p.guard ? tables : 0));
  need(p.ws_floats == want, "ws_floats is not what the form needs");
  if (p.ws_floats && p.ws_floats <= g_ws.size()) {
    ++g_carved;
    const AttnTables t = attention_tables(p, g_ws.data());
    const float* order[] = {t.wq, t.wk, t.wv, t.q_tab, t.p_tab, t.zero_tab, t.qk_inv, t.k_scale, t.k_inv, t.pv_inv, t.v_scale, t.v_inv, t.q_scale};
    const size_t sizes[] = {n * T * C, n * T * C, n * T * C, n * C, n * T, n * Z, n, n, n, n, n, n, n};
    size_t at = 0;
    bool ok = true;
    for (int i = 0; i < 13; ++i)
      if (order[i]) {
        ok = ok && order[i] == g_ws.data() + at;
        at += sizes[i];
      }
    need(ok && at + 64 == p.ws_floats, "carve: a table overlaps its neighbour or leaves the workspace");
    need((t.wq != nullptr) == flash && (t.wk != nullptr) == (flash || conv) && (t.wv != nullptr) == (flash || conv) && (t.q_scale != nullptr) == !conv &&
             t.q_tab && t.p_tab && t.zero_tab && t.qk_inv && t.k_scale && t.k_inv && t.pv_inv && t.v_scale && t.v_inv,
         "carve: the tables the form reads");
  }
  need(p.scores_floats == (flash ? 0 : (size_t)p.group * T * T) && (p.scores_floats == 0) == flash, "scores_floats");
  need(p.out_stats == !flash, "out_stats");
  need(flash == attention_flash_applicable((int)T, C, p.terms), "flash form and its rule disagree");
  need(!flash || (C == 384 && T % ATTN_FLASH_TILE == 0 && p.terms != 0), "flash form off its kernel's shape");
  const bool tail = conv && N % p.group != 0;
  g_tail += tail;
  need((p.qk[1].kernel != CONV_NONE) == tail && (p.pv[1].kernel != CONV_NONE) == tail, "plans of the short last group");
  need((p.qk[0].kernel != CONV_NONE) == conv && (p.pv[0].kernel != CONV_NONE) == conv, "GEMM plans off the conv form");
  if (conv) {
    need((long long)N * (long long)T > 1024 && p.terms != 0, "conv form on a sparse or exact-fp32 launch");
    for (int g = 0; g <= (tail ? 1 : 0); ++g)
      need(one_image_pipeline(p.qk[g], (int)T) && one_image_pipeline(p.pv[g], (int)T), "conv form: a GEMM is no pipeline plan with one image per pixel tile");
  }
  need(small || (!p.split_qk && !p.split_pv && !p.guard), "short-sequence flags off its form");
  need(!p.split_pv || (p.split_qk && T % 32 == 0), "split_pv without whole 32-chunks of T");
  need(!p.split_qk || (C % 32 == 0 && p.terms != 0), "split_qk without whole 32-chunks of C");
  need(p.guard == p.split_qk, "range guard and split S disagree");
}

int precision_of(const char* s) {
  for (int i = 0; i < 5; ++i)
    if (std::strcmp(s, PRECISIONS[i]) == 0) return i;
  return -1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--case") == 0) {
    const int prec = argc == 7 ? precision_of(argv[6]) : -1;
    if (prec < 0) {
      std::fprintf(stderr, "usage: attn_plan_check --case N H W C fp32|f16x3|f16|f16mx|bf16\n");
      return 2;
    }
    const int N = std::atoi(argv[2]), H = std::atoi(argv[3]), W = std::atoi(argv[4]), C = std::atoi(argv[5]);
    if (N < 1 || H < 1 || W < 1 || C < 1) return 2;
    const AttnPlan p = plan_attention(N, H, W, C, prec);
    const long long T = (long long)H * W;
    std::printf("form %s terms %d group %d passes %d tail %d split_qk %d split_pv %d guard %d workgroups %lld scores_floats %zu ws_floats %zu\n", FORMS[p.form],
                p.terms, p.group, (N + p.group - 1) / p.group, N % p.group, (int)p.split_qk, (int)p.split_pv, (int)p.guard,
                p.form == ATTN_FLASH ? N * (T / ATTN_FLASH_TILE) : 0ll, p.scores_floats, p.ws_floats);
    return 0;
  }
  // the (H, W) of every network level of a 64x64 .. 128x256 input, and the shapes of the tests
  std::set<std::pair<int, int>> maps;
  for (auto in : {std::make_pair(64, 64), std::make_pair(64, 128), std::make_pair(128, 128), std::make_pair(128, 256)})
    for (int ds = 1; ds <= 32; ds *= 2) maps.insert({in.first / ds, in.second / ds});
  for (auto m : {std::make_pair(32, 32), std::make_pair(24, 48), std::make_pair(16, 32), std::make_pair(16, 16), std::make_pair(8, 4), std::make_pair(4, 4),
                 std::make_pair(4, 8), std::make_pair(24, 32), std::make_pair(32, 40), std::make_pair(32, 48), std::make_pair(28, 64), std::make_pair(32, 34),
                 std::make_pair(32, 64), std::make_pair(6, 10), std::make_pair(7, 9)})
    maps.insert(m);
  for (int precision = PREC_FP32; precision <= PREC_BF16; ++precision)
    for (int N = 1; N <= 257; ++N)
      for (auto m : maps)
        for (int C = 32; C <= 768; C += 32) check(N, m.first, m.second, C, precision);
  std::printf("%lld plans over %zu maps: %lld short-sequence, %lld conv-pipeline (%lld with a short last group), %lld single-kernel; %lld carved; %lld violations\n",
              g_cases, maps.size(), g_form[ATTN_SMALL], g_form[ATTN_CONV], g_tail, g_form[ATTN_FLASH], g_carved, g_bad);
  std::printf("digest %016llx\n", (unsigned long long)g_digest);
  return g_bad == 0 ? 0 : 1;
}

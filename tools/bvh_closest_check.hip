// Stand-alone host check of the closest-hit walk: builds the BVH of six meshes with the library's own builder and runs bvh_closest against
// brute_closest (csrc/bvh.h, the code the kernels compile) for seeded rays; passes when every ray gives the same face and the same t, u, v
// bits, and bvh_occluded / brute_occluded the same answer as "a face was hit".  Host code only, meant for the sanitizers:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/bvh_closest_check.hip -o bvh_closest_check && ./bvh_closest_check [rays per family]
//
// No HIP call is made: it needs no GPU.  (bvh.hip is included whole, for the builder: its kernels are compiled for the device as well and never launched.)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../drmnet_amd/csrc/bvh.hip"

namespace drm {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
const char* last_error() { return g_error.c_str(); }
}  // namespace drm

namespace {

struct Mesh {
  const char* name;
  std::vector<float> p;
  std::vector<int32_t> f;
};

using Rng = std::mt19937_64;
float uni(Rng& g, float a, float b) { return std::uniform_real_distribution<float>(a, b)(g); }
float gauss(Rng& g) { return std::normal_distribution<float>(0.0f, 1.0f)(g); }

// F random triangles in the cube of side 1.8; `bad` adds the faces a builder must leave out
Mesh soup(const char* name, int F, uint64_t seed, bool bad) {
  Rng g(seed);
  Mesh m{name, {}, {}};
  for (int k = 0; k < F; ++k) {
    const float c[3] = {uni(g, -0.8f, 0.8f), uni(g, -0.8f, 0.8f), uni(g, -0.8f, 0.8f)};
    for (int v = 0; v < 3; ++v)
      for (int a = 0; a < 3; ++a) m.p.push_back(c[a] + uni(g, -0.1f, 0.1f));
    for (int v = 0; v < 3; ++v) m.f.push_back(3 * k + v);
  }
  if (bad && F > 20) {
    const int V = 3 * F;
    const int32_t rep[] = {30, 30, 31, 33, 34, 33};
    std::memcpy(&m.f[30], rep, sizeof(rep));  // faces 10, 11: a repeated vertex
    const float col[] = {0.25f, 0.5f, -0.125f, 0.5f, 0.5f, -0.125f, 0.375f, 0.5f, -0.125f};
    std::memcpy(&m.p[3 * 36], col, sizeof(col));  // face 12: collinear
    m.f[39] = -1;                                 // face 13
    m.f[43] = V;                                  // face 14
    m.p[3 * 45] = std::numeric_limits<float>::infinity();
    m.p[3 * 49 + 1] = std::numeric_limits<float>::quiet_NaN();
  }
  return m;
}

// a lat-long sphere of radius r about c, appended
void add_sphere(Mesh& m, float r, const float c[3], int rows, int cols) {
  const int base = (int)m.p.size() / 3;
  for (int i = 0; i <= rows; ++i)
    for (int j = 0; j < cols; ++j) {
      const float th = 3.14159265f * (float)i / (float)rows, ps = 6.2831853f * (float)j / (float)cols;
      m.p.push_back(c[0] + r * std::sin(th) * std::cos(ps));
      m.p.push_back(c[1] + r * std::cos(th));
      m.p.push_back(c[2] + r * std::sin(th) * std::sin(ps));
    }
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      const int a = base + i * cols + j, b = base + i * cols + (j + 1) % cols, c2 = a + cols, d = b + cols;
      const int32_t t[] = {a, b, c2, b, d, c2};  // (the polar rows hold zero-area faces: the builder leaves them out)
      m.f.insert(m.f.end(), t, t + 6);
    }
}

Mesh two_spheres() {
  Mesh m{"two_spheres", {}, {}};
  const float o[3] = {0, 0, 0}, b[3] = {0.40f, 0.35f, 0.30f};
  add_sphere(m, 0.55f, o, 10, 16);
  add_sphere(m, 0.22f, b, 5, 8);
  return m;
}

// the exact case: coordinates in 1/64, shared edges and a duplicated face
Mesh lattice() {
  Mesh m{"lattice", {}, {}};
  const int t[6][9] = {{0, -32, 16, 32, 0, 16, 0, 32, 16},     {0, -32, 16, 0, 32, 16, -32, 0, 16},     {-64, -64, -32, 64, -64, -32, 0, 64, -32},
                       {-16, -48, 48, 48, -48, 48, 16, -16, 40}, {-16, -48, 48, 48, -48, 48, 16, -16, 40}, {40, 40, -8, 40, 56, 24, 56, 40, 8}};
  for (auto& tri : t)
    for (int k = 0; k < 9; ++k) m.p.push_back((float)tri[k] / 64.0f);
  for (int k = 0; k < 18; ++k) m.f.push_back(k);
  return m;
}

uint32_t bits(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return b;
}

long long g_rays = 0, g_hits = 0, g_bad = 0;

void check(const Mesh& m, const drm::MeshRef& ref, const drm::BvhView& tree, const drm::Ray& r, int32_t ex) {
  const drm::Hit a = drm::bvh_closest(ref, tree, r, ex), b = drm::brute_closest(ref, r, ex);
  const bool oa = drm::bvh_occluded(ref, tree, r, ex), ob = drm::brute_occluded(ref, r, ex);
  ++g_rays;
  g_hits += b.face >= 0;
  if (a.face != b.face || bits(a.t) != bits(b.t) || bits(a.u) != bits(b.u) || bits(a.v) != bits(b.v) || oa != ob || ob != (b.face >= 0)) {
    if (++g_bad <= 10)
      std::printf("MISMATCH %s: o (%a %a %a) d (%a %a %a) ex %d: tree face %d t %a, brute face %d t %a, occluded %d / %d\n", m.name, r.o[0], r.o[1],
                  r.o[2], r.d[0], r.d[1], r.d[2], ex, a.face, a.t, b.face, b.t, (int)oa, (int)ob);
  }
}

void run(const Mesh& m, int n, uint64_t seed) {
  const long long V = (long long)m.p.size() / 3, F = (long long)m.f.size() / 3;
  std::vector<char> blob(drm::mesh_bvh_bytes(F));
  if (drm::mesh_bvh_build(m.p.data(), m.f.data(), V, F, blob.data(), blob.size()) != DRM_OK) {
    std::printf("%s: build failed: %s\n", m.name, drm::last_error());
    ++g_bad;
    return;
  }
  const drm::MeshRef ref{m.p.data(), m.f.data(), V, F};
  const drm::BvhView tree = drm::bvh_view(blob.data());
  Rng g(seed);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), den = 1e-41f;
  const float odd[] = {inf, -inf, nan, den, -den, 0.0f, -0.0f, 3e38f, 1e-30f};
  const long long before = g_rays, hits_before = g_hits;
  for (int k = 0; k < n; ++k) {
    drm::Ray r;
    int32_t ex = -1;
    // 0: random
    for (int a = 0; a < 3; ++a) r.o[a] = uni(g, -1, 1), r.d[a] = gauss(g);
    check(m, ref, tree, r, ex);
    // 1: one or two direction components exactly zero
    r.d[g() % 3] = 0.0f;
    if (k & 1) r.d[g() % 3] = 0.0f;
    check(m, ref, tree, r, ex);
    // 2: grid-aligned: origins in 1/32, integer directions up to 4, a rotating exclusion
    for (int a = 0; a < 3; ++a) r.o[a] = (float)((int)(g() % 65) - 32) / 32.0f, r.d[a] = (float)((int)(g() % 9) - 4);
    check(m, ref, tree, r, (int32_t)(k % 7) - 1);
    // 3: origin on a face (a vertex, an edge midpoint, an inner point), that face excluded or not; 4: grazing that face's plane
    const long long gf = (long long)(g() % (uint64_t)F);
    const int32_t* idx = &m.f[3 * gf];
    if (idx[0] >= 0 && idx[0] < V && idx[1] >= 0 && idx[1] < V && idx[2] >= 0 && idx[2] < V) {
      float w[3] = {uni(g, 0, 1), uni(g, 0, 1), uni(g, 0, 1)};
      if (k % 3 == 0) w[0] = 1, w[1] = w[2] = 0;
      if (k % 3 == 1) w[0] = w[1] = 0.5f, w[2] = 0;
      const float ws = w[0] + w[1] + w[2];
      for (int a = 0; a < 3; ++a) {
        r.o[a] = (w[0] * m.p[3 * idx[0] + a] + w[1] * m.p[3 * idx[1] + a] + w[2] * m.p[3 * idx[2] + a]) / ws;
        r.d[a] = gauss(g);
      }
      check(m, ref, tree, r, (k & 1) ? (int32_t)gf : -1);
      const float s1 = gauss(g), s2 = gauss(g), eps = (k % 4 == 0) ? 0.0f : std::ldexp(gauss(g), -(int)(g() % 24));
      for (int a = 0; a < 3; ++a) {
        r.o[a] = uni(g, -1, 1);
        r.d[a] = s1 * (m.p[3 * idx[1] + a] - m.p[3 * idx[0] + a]) + s2 * (m.p[3 * idx[2] + a] - m.p[3 * idx[0] + a]) + eps * gauss(g);
      }
      if (k & 2)
        for (int a = 0; a < 3; ++a) r.o[a] = m.p[3 * idx[k % 3] + a] - (1.0f + uni(g, 0, 1)) * r.d[a];  // ... aimed at the face from outside
      check(m, ref, tree, r, -1);
    }
    // 5: infinite, NaN, denormal and huge components
    for (int a = 0; a < 3; ++a) r.o[a] = uni(g, -1, 1), r.d[a] = gauss(g);
    (g() & 1 ? r.o : r.d)[g() % 3] = odd[g() % 9];
    if (k % 5 == 0) r.d[g() % 3] = odd[g() % 9];
    check(m, ref, tree, r, ex);
  }
  std::printf("%-12s %6lld faces, %8lld rays, %5.1f %% hit\n", m.name, F, g_rays - before, 100.0 * (double)(g_hits - hits_before) / (double)(g_rays - before));
}

}  // namespace

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 10000;
  const Mesh meshes[] = {soup("soup", 2000, 7, true), two_spheres(), soup("single", 1, 3, false), soup("five", 5, 4, false), lattice(),
                         soup("dense", 20000, 9, false)};
  uint64_t seed = 100;
  for (const Mesh& m : meshes) run(m, n, seed++);
  std::printf("%lld rays, %lld mismatches\n", g_rays, g_bad);
  return g_bad == 0 ? 0 : 1;
}

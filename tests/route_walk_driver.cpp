// The checked host walk of csrc/densemap_route_core.hpp (dm_route_walk, behind loamx_grid_route_trace and loamx_route3_trace) for both
// kinds, over hand-made fields: a valid one and the four refusals.  Stand-alone and host only (no device is touched), so that it can be
// built with -fsanitize=address,undefined: every output block has exactly the room the walk may use.
// tests/test_densemap_route_walk_cpu.py builds and runs it.  Prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include "densemap_route_core.hpp"
#include <cstdio>
#include <string>
#include <vector>

using namespace loamx;

static int checks = 0, failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    checks++;                                                          \
    if (!(cond)) {                                                     \
      failures++;                                                      \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
    }                                                                  \
  } while (0)

template <class K> struct Field {
  uint32_t nx, ny, nz;
  std::vector<loamx_route_cell> f;
  Field(uint32_t nx_, uint32_t ny_, uint32_t nz_) : nx(nx_), ny(ny_), nz(nz_), f((size_t)nx_ * ny_ * nz_, {LOAMX_ROUTE_UNREACHABLE, K::NONE}) {}
  loamx_route_cell& at(uint32_t x, uint32_t y, uint32_t z) { return f[((size_t)z * ny + y) * nx + x]; }
  // the walk into a block of exactly DIM * capacity words, each 0xdeadbeef before
  uint32_t walk(std::vector<uint32_t> start, uint32_t capacity, std::vector<uint32_t>& out) {
    out.assign((size_t)K::DIM * capacity, 0xdeadbeefu);
    return dm_route_walk<K>(f.data(), nx, ny, nz, start.data(), capacity ? out.data() : nullptr, capacity);
  }
  // the walk must be refused with `message` and leave nothing written
  void refused(std::vector<uint32_t> start, const std::string& message) {
    std::vector<uint32_t> out;
    std::string got = "(no error)";
    int code = 0;
    try {
      walk(start, 4u, out);
    } catch (const Error& e) {
      got = e.what();
      code = e.code;
    }
    EXPECT(got == message);
    EXPECT(code == LOAMX_E_INVALID);
    for (uint32_t v : out) EXPECT(v == 0xdeadbeefu);
    if (got != message) fprintf(stderr, "  got \"%s\", wanted \"%s\"\n", got.c_str(), message.c_str());
  }
};

// the direction of K whose move is (dx, dy, dz)
template <class K> static uint32_t dir(int dx, int dy, int dz) {
  for (uint32_t d = 0; d < K::GOAL; d++) {
    int a, b, c;
    K::move(d, a, b, c);
    if (a == dx && b == dy && c == dz) return d;
  }
  return K::NONE;
}

// a tuple of K from (x, y, z)
template <class K> static std::vector<uint32_t> tup(uint32_t x, uint32_t y, uint32_t z) {
  return K::DIM == 3 ? std::vector<uint32_t>{x, y, z} : std::vector<uint32_t>{x, z};
}

template <class K> static void run_kind() {
  const uint32_t ny = K::DIM == 3 ? 2u : 1u, ty = ny - 1u;   // (the far corner is (2, ty, 1))
  const std::string none_text = K::DIM == 3 ? "27" : "9";
  EXPECT(dir<K>(-1, 0, 0) < K::GOAL && dir<K>(-1, -(int)ty, -1) < K::GOAL && dir<K>(0, 0, -1) < K::GOAL);
  // 3 x ny x 2: the goal at the origin, two cells in a row towards it, the far corner one diagonal step from (1, 0, 0)
  Field<K> F(3, ny, 2);
  F.at(0, 0, 0) = {0u, K::GOAL};
  F.at(1, 0, 0) = {10u, dir<K>(-1, 0, 0)};
  F.at(2, 0, 0) = {20u, dir<K>(-1, 0, 0)};
  F.at(0, 0, 1) = {10u, dir<K>(0, 0, -1)};
  F.at(2, ty, 1) = {24u, dir<K>(-1, -(int)ty, -1)};
  std::vector<uint32_t> out;
  // the whole route, a truncated one, the length alone, the goal itself, an unreachable start, a start outside
  EXPECT(F.walk(tup<K>(2, ty, 1), 3u, out) == 3u);
  std::vector<uint32_t> want;
  for (const auto& t : {tup<K>(2, ty, 1), tup<K>(1, 0, 0), tup<K>(0, 0, 0)}) want.insert(want.end(), t.begin(), t.end());
  EXPECT(out == want);
  EXPECT(F.walk(tup<K>(2, ty, 1), 2u, out) == 3u);
  EXPECT(out == std::vector<uint32_t>(want.begin(), want.begin() + 2 * K::DIM));
  EXPECT(F.walk(tup<K>(2, ty, 1), 0u, out) == 3u);
  EXPECT(F.walk(tup<K>(0, 0, 0), 1u, out) == 1u && out == tup<K>(0, 0, 0));
  EXPECT(F.walk(tup<K>(1, 0, 1), 2u, out) == 0u && out[0] == 0xdeadbeefu);
  EXPECT(F.walk(tup<K>(3, 0, 0), 2u, out) == 0u && out[0] == 0xdeadbeefu);
  EXPECT(F.walk(tup<K>(0, 0, 2), 2u, out) == 0u && out[0] == 0xdeadbeefu);
  if (K::DIM == 3) EXPECT(F.walk(tup<K>(0, 2, 0), 2u, out) == 0u && out[0] == 0xdeadbeefu);
  // the refusals, each two steps into a route, so that the first pass has something it must not have written
  {
    Field<K> G = F;
    G.at(1, 0, 0).next = K::NONE + 1u;
    G.refused(tup<K>(2, 0, 0), "field: a next above " + none_text);
  }
  {
    Field<K> G = F;
    G.at(0, 0, 0) = {5u, dir<K>(-1, 0, 0)};   // (x wraps below 0)
    G.refused(tup<K>(2, 0, 0), "field: a step leaves the window");
    G.at(0, 0, 0) = {5u, dir<K>(0, 0, -1)};
    G.refused(tup<K>(2, 0, 0), "field: a step leaves the window");
  }
  {
    Field<K> G = F;
    G.at(1, 0, 0).cost = 20u;   // (equal to the cost of the cell that steps onto it)
    G.refused(tup<K>(2, 0, 0), "field: a step to a cell whose cost is not strictly smaller");
    G.at(1, 0, 0) = {10u, dir<K>(1, 0, 0)};   // (a loop would never end: the step back is to a larger cost)
    G.refused(tup<K>(2, 0, 0), "field: a step to a cell whose cost is not strictly smaller");
  }
  {
    Field<K> G = F;
    G.at(0, 0, 0) = {0u, K::NONE};
    G.refused(tup<K>(2, 0, 0), "field: the route ends on a cell that is no goal");
  }
}

int main() {
  run_kind<DmRouteGrid>();
  run_kind<DmRouteVol>();
  if (failures) {
    fprintf(stderr, "%d of %d checks failed\n", failures, checks);
    return 1;
  }
  printf("ok %d\n", checks);
  return 0;
}

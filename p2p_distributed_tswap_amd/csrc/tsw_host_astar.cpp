// tsw_host_astar.cpp — exact A* next hop on a host core; plain C++ (no HIP, no device): see
// tsw_host_astar.h. The search itself is tsw_astar.h's astar_one, compiled here for the host.
#include "tsw_host_astar.h"

#include <algorithm>
#include <new>

#include "tsw_astar.h"
#include "tswap.h"

namespace tsw {

void host_nbmask(const uint8_t* cells, uint32_t w, uint32_t h, uint8_t* out) {
  auto fr = [&](uint32_t x, uint32_t y) { return cells[(size_t)y * w + x] != '@'; };
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      uint8_t m = 0;
      if (fr(x, y)) {
        m = NB_FREE;
        if (y + 1 < h && fr(x, y + 1)) m |= 1;
        if (x + 1 < w && fr(x + 1, y)) m |= 2;
        if (y > 0 && fr(x, y - 1)) m |= 4;
        if (x > 0 && fr(x - 1, y)) m |= 8;
      }
      out[(size_t)y * w + x] = m;
    }
}

uint8_t host_next_hop(HostAstar& S, const uint8_t* nbmask, uint32_t w, uint32_t h, uint32_t v, uint32_t goal) {
  const uint32_t ncell = w * h;
  if (S.gs.size() != ncell) {
    S.gs.assign(ncell, 0u);
    S.heap.resize(4u * (size_t)ncell + 8u);
    S.tag = 0;
  }
  if (++S.tag > 1023u) {  // 10-bit tags: wipe the stamps when they wrap
    std::fill(S.gs.begin(), S.gs.end(), 0u);
    S.tag = 1;
  }
  DevGrid G{};
  G.W = w;
  G.H = h;
  G.ncell = ncell;
  G.nbmask = nbmask;
  int32_t len = 0;
  return astar_one(G, v, goal, S.tag, S.heap.data(), (uint32_t)S.heap.size(), S.gs.data(), &len, nullptr);
}

}  // namespace tsw

extern "C" int tsw_host_next_hop_codes(const uint8_t* cells, uint32_t w, uint32_t h, const uint32_t* start,
                                       const uint32_t* goal, uint32_t k, uint8_t* code) {
  using namespace tsw;
  if (!cells || w == 0 || h == 0 || w > MAX_WH || h > MAX_WH || (uint64_t)w * h > MAX_CELLS) return TSW_EINVAL;
  if (k && (!start || !goal || !code)) return TSW_EINVAL;
  try {
    std::vector<uint8_t> nb((size_t)w * h);
    host_nbmask(cells, w, h, nb.data());
    HostAstar S;
    for (uint32_t i = 0; i < k; ++i) {
      if (start[i] >= w * h || goal[i] >= w * h || !(nb[start[i]] & NB_FREE) || !(nb[goal[i]] & NB_FREE))
        return TSW_EINVAL;
      code[i] = host_next_hop(S, nb.data(), w, h, start[i], goal[i]);
    }
  } catch (const std::bad_alloc&) {
    return TSW_ENOMEM;
  }
  return TSW_OK;
}

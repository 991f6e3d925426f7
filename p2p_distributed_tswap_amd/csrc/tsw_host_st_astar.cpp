// tsw_host_st_astar.cpp — astar_with_reservation (a_star.rs:32-112) on a host core; plain C++ (no HIP, no
// device): tsw_host_astar_reserved, the twin of K9 (tsw_st_astar.hip). The heap order is tsw_astar.h's
// heap_sift_up / heap_pop compiled for the host, the reservation set and the visited table are
// tsw_st_astar.h's — shared with the kernel, so a mistake in the key packing or in an edge's direction would be
// common to both: the implementation that shares nothing is the Python model (tests/st_astar_model.py), and both
// are tested against it. The search loop below is written out serially, one successor after the other, as the
// reference has it.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "tsw_astar.h"
#include "tsw_st_astar.h"
#include "tswap.h"

namespace tsw {

namespace {

struct HostStAstar {
  std::vector<uint64_t> vis, heap;
  uint32_t vis_mask = 0, tag = 0;
};

// One query. path: room for st_path_room entries. Returns the status; *len = path entries (0 unless found).
uint32_t st_search_host(HostStAstar& S, const uint8_t* cells, uint32_t W, uint32_t H, const StResSet& R, uint32_t start,
                        uint32_t goal, uint32_t st, uint32_t max_time, uint32_t max_nodes, uint32_t* path, uint32_t room,
                        uint32_t* len, uint32_t* pops_out) {
  const uint32_t ncell = W * H;
  const uint32_t gx = goal % W, gy = goal / W;
  auto man = [&](uint32_t x, uint32_t y) { return (x > gx ? x - gx : gx - x) + (y > gy ? y - gy : gy - y); };
  if (++S.tag > ST_TAG_MAX) {  // the tags wrapped: wipe
    std::fill(S.vis.begin(), S.vis.end(), 0ull);
    S.tag = 1;
  }
  uint64_t* Hp = S.heap.data();
  uint32_t hlen = 1, pushes = 1, pops = 0;
  Hp[0] = mk_entry(st + man(start % W, start / W), st, start % W, start / W);
  *len = 0;
  uint32_t status = TSW_SP_NONE;
  while (hlen > 0) {
    const uint64_t e = heap_pop(Hp, hlen);
    const uint32_t f = (uint32_t)(e >> 43), g = (uint32_t)(e >> 22) & 0x1FFFFFu;
    const uint32_t x = (uint32_t)(e >> 11) & 0x7FFu, y = (uint32_t)e & 0x7FFu;
    if (f > max_time) break;  // the horizon
    ++pops;
    const uint32_t c = y * W + x;
    if (c == goal) {
      uint32_t dt = g - st, cur = c;
      status = dt < room ? (uint32_t)TSW_SP_FOUND : ST_SP_INTERNAL;
      if (status == TSW_SP_FOUND) {
        *len = dt + 1u;
        path[dt] = cur;
        while (dt > 0) {
          bool found;
          const uint32_t slot = st_vis_find(S.vis.data(), S.vis_mask, S.tag, (uint64_t)dt * ncell + cur, &found);
          if (!found) {
            status = ST_SP_INTERNAL;
            *len = 0;
            break;
          }
          const uint32_t d = (uint32_t)S.vis[slot] & 7u;
          const uint32_t px = cur % W - st_dx(d), py = cur / W - st_dy(d);
          if (px >= W || py >= H) {  // a direction that leaves the grid: never written by the search
            status = ST_SP_INTERNAL;
            *len = 0;
            break;
          }
          cur = py * W + px;
          path[--dt] = cur;
        }
      }
      break;
    }
    const uint32_t nt = g + 1u;
    if (st_res_has(R.data(), R.mask, st_res_key(nt, c, ST_KIND_NODE, ncell))) continue;  // (pos, nt) reserved
    bool full = false;
    for (uint32_t d = 0; d < ST_NDIR; ++d) {
      const uint32_t nx = x + st_dx(d), ny = y + st_dy(d);
      if (nx >= W || ny >= H) continue;
      const uint32_t nc = ny * W + nx;
      if (cells[nc] == '@') continue;
      if (st_res_has(R.data(), R.mask, st_res_key(nt, nc, ST_KIND_NODE, ncell))) continue;
      if (st_res_has(R.data(), R.mask, st_res_key(nt, c, d, ncell))) continue;
      bool seen;
      const uint32_t slot = st_vis_find(S.vis.data(), S.vis_mask, S.tag, (uint64_t)(nt - st) * ncell + nc, &seen);
      if (seen) continue;
      if (pushes == max_nodes || slot > S.vis_mask) {
        full = true;
        break;
      }
      S.vis[slot] = st_vis_word(S.tag, (uint64_t)(nt - st) * ncell + nc, d);
      heap_sift_up(Hp, hlen, mk_entry(nt + man(nx, ny), nt, nx, ny));
      ++hlen;
      ++pushes;
    }
    if (full) {
      status = TSW_SP_CAPACITY;
      break;
    }
  }
  *pops_out = pops;
  return status;
}

}  // namespace

}  // namespace tsw

extern "C" int tsw_host_astar_reserved(const uint8_t* cells, uint32_t w, uint32_t h, const uint32_t* start,
                                       const uint32_t* goal, const uint32_t* start_time, uint32_t k,
                                       const tsw_node_res* node_res, uint32_t n_node, const tsw_edge_res* edge_res,
                                       uint32_t n_edge, uint32_t max_time, uint32_t max_nodes, uint32_t* path_off,
                                       uint32_t* path, uint32_t path_cap, uint32_t* status, uint32_t* pops,
                                       uint32_t* total) {
  using namespace tsw;
  if (!cells || w == 0 || h == 0 || w > MAX_WH || h > MAX_WH || (uint64_t)w * h > MAX_CELLS) return TSW_EINVAL;
  if (max_time > ST_MAX_TIME || max_nodes == 0) return TSW_EINVAL;
  if (k && (!start || !goal || !start_time || !status)) return TSW_EINVAL;
  if (!path_off || !total || (n_node && !node_res) || (n_edge && !edge_res) || (path_cap && !path)) return TSW_EINVAL;
  const uint32_t ncell = w * h;
  for (uint32_t i = 0; i < k; ++i)
    if (start[i] >= ncell || goal[i] >= ncell || cells[start[i]] == '@' || cells[goal[i]] == '@' ||
        start_time[i] > ST_MAX_TIME)
      return TSW_EINVAL;
  static_assert(sizeof(tsw_node_res) == sizeof(StNode) && sizeof(tsw_edge_res) == sizeof(StEdge), "same layout");
  try {
    StResSet R;
    st_build_reservations(reinterpret_cast<const StNode*>(node_res), n_node, reinterpret_cast<const StEdge*>(edge_res),
                          n_edge, w, h, max_time, &R);
    const uint32_t eff = st_eff_nodes(ncell, max_time, max_nodes);
    if (st_vis_slots(eff) > ST_SLOTS_MAX) return TSW_ENOMEM;  // the table's mask is a 32-bit word
    HostStAstar S;
    S.vis.assign((size_t)st_vis_slots(eff), 0ull);
    S.vis_mask = (uint32_t)(S.vis.size() - 1u);
    S.heap.resize((size_t)eff + 1u);
    std::vector<uint32_t> all, one;  // the paths go to the caller only once the total is known to fit
    uint64_t tot = 0;
    for (uint32_t i = 0; i < k; ++i) {
      const uint32_t room = st_path_room(start_time[i], max_time, eff);
      one.resize(room);
      uint32_t len = 0, np = 0;
      const uint32_t s = st_search_host(S, cells, w, h, R, start[i], goal[i], start_time[i], max_time, eff, one.data(),
                                        room, &len, &np);
      if (s == ST_SP_INTERNAL) return TSW_EHIP;
      status[i] = s;
      if (pops) pops[i] = np;
      path_off[i] = (uint32_t)tot;
      tot += len;
      if (tot > 0xFFFFFFFFull) return TSW_EOVERFLOW;
      if (tot <= path_cap) all.insert(all.end(), one.begin(), one.begin() + len);
    }
    path_off[k] = (uint32_t)tot;
    *total = (uint32_t)tot;
    if (tot > path_cap) return TSW_EOVERFLOW;
    if (tot) std::memcpy(path, all.data(), (size_t)tot * 4u);
  } catch (const std::bad_alloc&) {
    return TSW_ENOMEM;
  }
  return TSW_OK;
}

// tsw_st_astar.h — K9: astar_with_reservation (a_star.rs:32-112) over (cell, time), what the kernel
// (tsw_st_astar.hip), its host side (tsw_st_astar_host.hip) and the host twin (tsw_host_st_astar.cpp, plain
// C++) share: the successor order, the reservation set and the visited table. The BinaryHeap order is
// tsw_astar.h's (mk_entry / heap_sift_up / heap_pop): TimeNode's Ord is AstarNode's.
//
// Reservation set: one open-addressing set of 64-bit keys for vertices and edges,
//   key = (t * ncell + cell) << 3 | kind,  kind 0..4: an edge leaving `cell` in direction kind at time t,
//                                          kind 5: the vertex (cell, t).
// An edge ((a, b), t) is stored from both ends (a in the direction of b, b in the direction of a), so the
// reference's two tests ((pos, np), nt) and ((np, pos), nt) are one lookup. Entries that can never match (a
// cell off the grid, a pair that is neither adjacent nor equal, t == 0 or t > max_time + 1) are dropped when
// the set is built: a successor's time is g + 1 with start_time <= g <= max_time.
//
// Visited table (one per running query, the owner alone touches it): open addressing over 64-bit words
//   tag:18 | key:43 | dir:3,  key = (t - start_time) * ncell + cell, dir = the direction the state was entered by
// — the parent is one time step back, so the direction is the whole came_from entry. tag names the query: a
// word with another tag is an empty slot, so a table is wiped once per 2^18 - 1 queries, not once per query.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "tsw_internal.h"

namespace tsw {

constexpr uint32_t ST_MAX_TIME = 1u << 20;  // max_time and start_time: f = g + h stays below 2^21 (mk_entry)
constexpr uint32_t ST_NDIR = 5u, ST_KIND_NODE = 5u;
constexpr uint32_t ST_TAG_BITS = 18u, ST_TAG_MAX = (1u << ST_TAG_BITS) - 1u;
constexpr uint64_t ST_RES_EMPTY = ~0ull;
constexpr uint64_t ST_SLOTS_MAX = 1ull << 31;  // slots of one table: the masks are 32-bit words
constexpr uint32_t ST_SP_INTERNAL = 3u;  // a came_from chain that does not reach the start: never expected

// successor d of (x, y), a_star.rs:40's order (1,0), (-1,0), (0,1), (0,-1), (0,0); unsigned wrap at 0 fails
// the caller's bound test
TSW_HD uint32_t st_dx(uint32_t d) { return d == 0u ? 1u : (d == 1u ? 0xFFFFFFFFu : 0u); }
TSW_HD uint32_t st_dy(uint32_t d) { return d == 2u ? 1u : (d == 3u ? 0xFFFFFFFFu : 0u); }

TSW_HD uint64_t st_mix(uint64_t k) {  // splitmix64's finalizer
  k ^= k >> 30;
  k *= 0xBF58476D1CE4E5B9ull;
  k ^= k >> 27;
  k *= 0x94D049BB133111EBull;
  return k ^ (k >> 31);
}

TSW_HD uint64_t st_res_key(uint32_t t, uint32_t cell, uint32_t kind, uint32_t ncell) {
  return (((uint64_t)t * ncell + cell) << 3) | kind;
}

// set == nullptr: no reservation at all. At most mask + 1 probes.
TSW_HD bool st_res_has(const uint64_t* set, uint32_t mask, uint64_t key) {
  if (!set) return false;
  uint32_t i = (uint32_t)st_mix(key) & mask;
  for (uint32_t n = 0; n <= mask; ++n) {
    const uint64_t s = set[i];
    if (s == key) return true;
    if (s == ST_RES_EMPTY) return false;
    i = (i + 1u) & mask;
  }
  return false;
}

TSW_HD uint64_t st_vis_word(uint32_t tag, uint64_t key, uint32_t dir) {
  return ((uint64_t)tag << 46) | (key << 3) | dir;
}

// The state's slot, or the first empty one of its probe sequence (*found tells which). At most mask + 1
// probes; a full table without the key gives *found = false and slot = mask + 1.
TSW_HD uint32_t st_vis_find(const uint64_t* tab, uint32_t mask, uint32_t tag, uint64_t key, bool* found) {
  const uint64_t want = ((uint64_t)tag << 43) | key;
  uint32_t i = (uint32_t)st_mix(key) & mask;
  *found = false;
  for (uint32_t n = 0; n <= mask; ++n) {
    const uint64_t s = tab[i];
    if ((s >> 3) == want) {
      *found = true;
      return i;
    }
    if ((uint32_t)(s >> 46) != tag) return i;
    i = (i + 1u) & mask;
  }
  return mask + 1u;
}

// The states a search can push: max_nodes beyond them buys nothing, and the tables are sized from this.
inline uint32_t st_eff_nodes(uint32_t ncell, uint32_t max_time, uint32_t max_nodes) {
  const uint64_t states = (uint64_t)ncell * ((uint64_t)max_time + 2u);
  return (uint32_t)(states < max_nodes ? states : max_nodes);
}
// visited-table slots of one query: a power of two, load factor <= 1/2 (64-bit: the caller checks the fit)
inline uint64_t st_vis_slots(uint32_t eff_nodes) {
  uint64_t s = 16;
  while (s < 2ull * eff_nodes) s <<= 1;
  return s;
}
// room of query i's path: a found path arrives by max_time, and every state on it but the start was pushed
inline uint32_t st_path_room(uint32_t start_time, uint32_t max_time, uint32_t eff_nodes) {
  if (start_time > max_time) return 1u;
  const uint32_t by_time = max_time - start_time + 1u;
  return by_time < eff_nodes ? by_time : eff_nodes;
}

struct StEdge {
  uint32_t from, to, t;
};
struct StNode {
  uint32_t cell, t;
};

// The reservation set of a call (host memory). Empty: set.empty(), mask 0.
struct StResSet {
  std::vector<uint64_t> set;
  uint32_t mask = 0;
  const uint64_t* data() const { return set.empty() ? nullptr : set.data(); }
};

inline void st_build_reservations(const StNode* node, uint32_t n_node, const StEdge* edge, uint32_t n_edge,
                                  uint32_t w, uint32_t h, uint32_t max_time, StResSet* out) {
  const uint32_t ncell = w * h;
  std::vector<uint64_t> keys;
  keys.reserve((size_t)n_node + 2u * (size_t)n_edge);
  auto t_ok = [&](uint32_t t) { return t >= 1u && t <= max_time + 1u; };
  for (uint32_t i = 0; i < n_node; ++i)
    if (node[i].cell < ncell && t_ok(node[i].t)) keys.push_back(st_res_key(node[i].t, node[i].cell, ST_KIND_NODE, ncell));
  for (uint32_t i = 0; i < n_edge; ++i) {
    const uint32_t a = edge[i].from, b = edge[i].to, t = edge[i].t;
    if (a >= ncell || b >= ncell || !t_ok(t)) continue;
    const uint32_t ax = a % w, bx = b % w;
    uint32_t da, db;  // the direction of b from a, and of a from b
    if (b == a) da = db = 4u;
    else if (b == a + 1u && bx == ax + 1u) da = 0u, db = 1u;
    else if (a == b + 1u && ax == bx + 1u) da = 1u, db = 0u;
    else if (b == a + w) da = 2u, db = 3u;
    else if (a == b + w) da = 3u, db = 2u;
    else continue;
    keys.push_back(st_res_key(t, a, da, ncell));
    if (b != a) keys.push_back(st_res_key(t, b, db, ncell));
  }
  out->set.clear();
  out->mask = 0;
  if (keys.empty()) return;
  uint64_t slots = 16;
  while (slots < 2ull * keys.size()) slots <<= 1;
  if (slots > ST_SLOTS_MAX) throw std::bad_alloc();  // refused like a set that does not fit: TSW_ENOMEM
  out->set.assign((size_t)slots, ST_RES_EMPTY);
  out->mask = (uint32_t)(slots - 1u);
  for (uint64_t key : keys) {
    uint32_t i = (uint32_t)st_mix(key) & out->mask;
    while (out->set[i] != ST_RES_EMPTY && out->set[i] != key) i = (i + 1u) & out->mask;
    out->set[i] = key;
  }
}

#if defined(__HIPCC__)
// ---- the kernels' arguments and launchers (tsw_st_astar.hip) ----------------------------------------
struct StAstarArgs {
  uint32_t W, H, ncell, Ww;
  const uint32_t* freebits;
  uint32_t k;                                  // queries of this launch
  const uint32_t *start, *goal, *start_time;   // k each
  const uint64_t* res;                         // reservation set (nullptr: none)
  uint32_t res_mask;
  uint32_t max_time, max_nodes;                // max_nodes: st_eff_nodes
  uint32_t nslots;                             // waves of the launch; wave s runs queries s, s + nslots, ...
  uint32_t wpb, hl, fb_lds;                    // waves per workgroup, LDS heap entries per wave, bitmap staged in LDS
  uint32_t tag0;                               // tag of a wave's first query; its j-th query has tag0 + j <= ST_TAG_MAX
  uint64_t* vis;                               // nslots tables of vis_mask + 1 words
  uint32_t vis_mask;
  uint64_t* gheap;                             // nslots overflow heaps of max_nodes entries
  const uint64_t* seg_off;                     // k + 1: query i's path room in seg
  uint32_t* seg;
  uint32_t *status, *pops, *len;               // k each
};
hipError_t launch_st_astar(const StAstarArgs& A, size_t lds, hipStream_t s);
// path[path_off[i] + j] = seg[seg_off[i] + j], j < len[i]
hipError_t launch_st_pack(uint32_t k, const uint64_t* seg_off, const uint32_t* seg, const uint32_t* path_off,
                          const uint32_t* len, uint32_t* path, hipStream_t s);
#endif

}  // namespace tsw

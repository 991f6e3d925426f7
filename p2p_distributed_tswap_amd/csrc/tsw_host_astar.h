// tsw_host_astar.h — the exact A* next hop on a host core (plain C++, no HIP): the same astar_one,
// heap_sift_up and heap_pop as the device (tsw_astar.h, __host__ __device__) run over the host copy of
// the neighbour masks. Used by the plan dispatch's host service (tsw_plan_host.hip: the calling thread
// answers the planner's needed pairs while k_plan runs) and by tsw_host_next_hop_codes.
#pragma once
#include <stdint.h>

#include <vector>

namespace tsw {

// Scratch of one serving thread: a dense tag-stamped g-score word per cell (tag:10 | label:2 | g:20,
// as the device's) and the BinaryHeap array. 4 * cells + 8 entries hold every push of one query (a cell
// is relaxed at most once per neighbour), so the heap cannot overflow.
struct HostAstar {
  std::vector<uint32_t> gs;
  std::vector<uint64_t> heap;
  uint32_t tag = 0;
};

// Neighbour masks of a grid (cells: h rows of w bytes, '@' = blocked): bit d = the neighbour in
// direction d (S, E, N, W) is free, NB_FREE = the cell is free. out: w * h bytes.
void host_nbmask(const uint8_t* cells, uint32_t w, uint32_t h, uint8_t* out);

// Next-hop code of get_path(v, goal): 0..3 = S, E, N, W, NH_STAY when v == goal or the goal is
// unreachable with no closer neighbour. v and goal are free cells of the grid.
uint8_t host_next_hop(HostAstar& S, const uint8_t* nbmask, uint32_t w, uint32_t h, uint32_t v, uint32_t goal);

}  // namespace tsw

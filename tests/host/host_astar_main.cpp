// Stand-alone driver of the host A* (csrc/tsw_host_astar.cpp) for a sanitizer build: compiled by
// tests/test_host_astar_sanitized.py with the host compiler and -fsanitize=address,undefined, together
// with the A* translation unit. Seeded grids (open, random obstacles, a 1 x N corridor, a split grid) and
// a few hundred seeded pairs each, through tsw_host_next_hop_codes; every code must be a legal move, and
// following the codes from a start must reach a reachable goal in a shortest number of steps (BFS).
#include <cstdint>
#include <cstdio>
#include <queue>
#include <vector>

#include "tswap.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 33) % n);
}

static std::vector<uint32_t> bfs(const std::vector<uint8_t>& cells, uint32_t w, uint32_t h, uint32_t goal) {
  std::vector<uint32_t> d((size_t)w * h, 0xFFFFFFFFu);
  std::queue<uint32_t> q;
  d[goal] = 0;
  q.push(goal);
  while (!q.empty()) {
    const uint32_t c = q.front();
    q.pop();
    const uint32_t x = c % w, y = c / w;
    const int64_t nb[4] = {y + 1 < h ? (int64_t)c + w : -1, x + 1 < w ? (int64_t)c + 1 : -1, y > 0 ? (int64_t)c - w : -1,
                           x > 0 ? (int64_t)c - 1 : -1};
    for (int64_t n : nb)
      if (n >= 0 && cells[(size_t)n] != '@' && d[(size_t)n] == 0xFFFFFFFFu) {
        d[(size_t)n] = d[c] + 1;
        q.push((uint32_t)n);
      }
  }
  return d;
}

static int run_grid(const char* name, const std::vector<uint8_t>& cells, uint32_t w, uint32_t h, uint32_t pairs) {
  std::vector<uint32_t> free_cells;
  for (uint32_t c = 0; c < w * h; ++c)
    if (cells[c] != '@') free_cells.push_back(c);
  if (free_cells.empty()) return 0;
  const int64_t step[5] = {(int64_t)w, 1, -(int64_t)w, -1, 0};
  for (uint32_t p = 0; p < pairs; ++p) {
    uint32_t cur = free_cells[rnd((uint32_t)free_cells.size())];
    const uint32_t goal = free_cells[rnd((uint32_t)free_cells.size())];
    const std::vector<uint32_t> d = bfs(cells, w, h, goal);
    const bool reach = d[cur] != 0xFFFFFFFFu;
    // a reachable goal: walk the whole path, one query per hop; otherwise one query (the fallback)
    for (uint32_t hops = 0; hops <= w * h; ++hops) {
      uint8_t code = 0xFF;
      if (tsw_host_next_hop_codes(cells.data(), w, h, &cur, &goal, 1, &code) != TSW_OK || code > 4) {
        fprintf(stderr, "%s: query (%u -> %u) failed, code %u\n", name, cur, goal, code);
        return 1;
      }
      if (cur == goal) {
        if (code != 4) return fprintf(stderr, "%s: start == goal gave code %u\n", name, code), 1;
        break;
      }
      const uint32_t x = cur % w, y = cur / w;
      if ((code == 0 && y + 1 >= h) || (code == 1 && x + 1 >= w) || (code == 2 && y == 0) || (code == 3 && x == 0))
        return fprintf(stderr, "%s: code %u leaves the grid at %u\n", name, code, cur), 1;
      const uint32_t nxt = (uint32_t)((int64_t)cur + step[code]);
      if (cells[nxt] == '@') return fprintf(stderr, "%s: code %u enters a blocked cell at %u\n", name, code, cur), 1;
      if (!reach) break;
      if (code == 4 || d[nxt] + 1 != d[cur])
        return fprintf(stderr, "%s: hop %u -> %u is not on a shortest path to %u\n", name, cur, nxt, goal), 1;
      cur = nxt;
    }
  }
  return 0;
}

int main() {
  int bad = 0;
  {
    std::vector<uint8_t> g(8 * 8, '.');
    bad |= run_grid("open8x8", g, 8, 8, 100);
  }
  for (uint32_t seed = 0; seed < 3; ++seed) {
    const uint32_t w = 17 + 6 * seed, h = 13 + 5 * seed;
    std::vector<uint8_t> g((size_t)w * h, '.');
    for (auto& c : g)
      if (rnd(100) < 22) c = '@';
    bad |= run_grid("random", g, w, h, 100);
  }
  {
    std::vector<uint8_t> g(41, '.');
    bad |= run_grid("corridor1x41", g, 41, 1, 60);
    bad |= run_grid("corridor41x1", g, 1, 41, 60);
  }
  {
    std::vector<uint8_t> g(9 * 5, '.');
    for (uint32_t y = 0; y < 5; ++y) g[y * 9 + 4] = '@';
    bad |= run_grid("split9x5", g, 9, 5, 60);
  }
  {
    // refused inputs: a blocked start, an off-grid goal, a null grid
    std::vector<uint8_t> g = {'.', '@', '.', '.'};
    uint32_t s = 1, t = 0, off = 9;
    uint8_t code = 0;
    if (tsw_host_next_hop_codes(g.data(), 2, 2, &s, &t, 1, &code) != TSW_EINVAL) bad |= 1;
    if (tsw_host_next_hop_codes(g.data(), 2, 2, &t, &off, 1, &code) != TSW_EINVAL) bad |= 1;
    if (tsw_host_next_hop_codes(nullptr, 2, 2, &t, &t, 1, &code) != TSW_EINVAL) bad |= 1;
  }
  if (bad) return 1;
  printf("host A* sanitizer run ok\n");
  return 0;
}

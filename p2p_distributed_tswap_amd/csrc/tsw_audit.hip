// tsw_audit.hip — K6: the audit of plan records (the definitions above tsw_audit_records in include/tswap.h).
// The records are agent-major; the per-agent facts want that layout, the conflicts of a column want its
// transpose. Two passes:
//
//   k_audit_rows     pass A, one workgroup per tile of AUD_TILE_AGENTS agents x AUD_TILE_COLS columns. A wave
//                    reads AUD_TILE_COLS consecutive records of one agent (lane = column, coalesced) and walks
//                    down the tile's agents, so a lane counts its column in registers: states, bad_state,
//                    moved, deliveries, jumps, off_map. The waves' counts meet in LDS and leave as one atomic
//                    per (tile, column, counter) that is not zero. Moves and deliveries of an agent are a wave
//                    ballot. Every record also becomes one word of the column-major transpose (tsw_audit.h:
//                    cell id, the unit step that led to it, "charged by pass A"), turned through an LDS tile.
//   k_audit_columns  pass B, columns strided over G workgroups, each with an occupancy table of one entry per
//                    cell, in LDS when it fits and in global scratch otherwise. Phase 1 of a column: every
//                    agent on the grid lowers its cell's entry to its index and adds its direction to the
//                    entry of the cell it left. Phase 2: an agent that is not its cell's entry is a
//                    colocation; one whose cell records the reverse of its own direction is a swap (some
//                    agent left its destination for its origin). Entries carry the workgroup's column tag, so
//                    the table is never cleared between columns. A column has one owner: its two counters
//                    are plain stores. Per-agent violation columns are counted here, pass A's bit included.
// First violations per kind are atomicMin on t << 32 | agent. No atomic decides an order: minima, sums and
// a set union.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tsw_audit.h"

namespace tsw {

namespace {

constexpr unsigned long long AUD_NONE = ~0ull;
constexpr uint32_t AUD_A_WAVES = AUD_A_BLOCK / 64u;
constexpr uint32_t AUD_A_NCNT = 9u;  // pass A's counters of a column: AUD_NCOL without colocations and swaps
static_assert(AUD_TILE_COLS == 64u, "pass A: one lane per column of the tile");
static_assert(AUD_TILE_AGENTS == 64u, "pass A: one lane per agent of the tile when the transpose is written");

__global__ __launch_bounds__(AUD_A_BLOCK) void k_audit_rows(AuditArgs A) {
  __shared__ uint32_t s_cid[AUD_TILE_COLS][AUD_TILE_AGENTS + 1];
  __shared__ uint32_t s_cnt[AUD_TILE_COLS][AUD_A_NCNT];
  __shared__ unsigned long long s_first[3];  // jump, off_map, bad_state
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i0 = blockIdx.x * AUD_TILE_AGENTS, t0 = blockIdx.y * AUD_TILE_COLS;
  const uint32_t t = t0 + lane;
  for (uint32_t k = threadIdx.x; k < AUD_TILE_COLS * AUD_A_NCNT; k += AUD_A_BLOCK) (&s_cnt[0][0])[k] = 0;
  if (threadIdx.x < 3) s_first[threadIdx.x] = AUD_NONE;
  __syncthreads();

  uint32_t c_st0 = 0, c_st1 = 0, c_st2 = 0, c_st3 = 0, c_bad = 0, c_moved = 0, c_deliv = 0, c_jump = 0, c_off = 0;
  unsigned long long f_jump = AUD_NONE, f_off = AUD_NONE, f_bad = AUD_NONE;
  for (uint32_t a = wave; a < AUD_TILE_AGENTS; a += AUD_A_WAVES) {
    const uint32_t i = i0 + a;
    if (i >= A.n) break;  // the same for the whole wave
    uint32_t word = AUD_CID_OFF;
    bool moved = false, deliv = false;
    if (t < A.T) {
      const unsigned long long* row = A.rec + (size_t)i * A.stride;
      const unsigned long long r = row[t];
      const uint32_t x = (uint32_t)r & 0xFFFFu, y = (uint32_t)(r >> 16) & 0xFFFFu, st = (uint32_t)(r >> 32) & 0xFFu;
      const bool on = x < A.W && y < A.H;
      const bool off = !on || !((A.freebits[(size_t)y * A.Ww + (x >> 5)] >> (x & 31u)) & 1u);
      const bool bad = st > 3u;
      bool jump = false;
      uint32_t dir = 0;  // 1 + AUD_DIR_*
      deliv = st == 2u;
      if (t > 0) {
        const unsigned long long p = row[t - 1];
        const uint32_t px = (uint32_t)p & 0xFFFFu, py = (uint32_t)(p >> 16) & 0xFFFFu, pst = (uint32_t)(p >> 32) & 0xFFu;
        const int dx = (int)x - (int)px, dy = (int)y - (int)py;
        const uint32_t dist = (uint32_t)(dx < 0 ? -dx : dx) + (uint32_t)(dy < 0 ? -dy : dy);
        moved = dist != 0;
        jump = dist > 1u;
        deliv = deliv && pst != 2u;
        if (dist == 1u && on && px < A.W && py < A.H)
          dir = 1u + (dx == 1 ? AUD_DIR_E : dx == -1 ? AUD_DIR_W : dy == 1 ? AUD_DIR_S : AUD_DIR_N);
      }
      c_st0 += st == 0u;
      c_st1 += st == 1u;
      c_st2 += st == 2u;
      c_st3 += st == 3u;
      c_bad += bad;
      c_moved += moved;
      c_deliv += deliv;
      c_jump += jump;
      c_off += off;
      const unsigned long long key = (unsigned long long)t << 32 | i;
      if (jump) f_jump = min(f_jump, key);
      if (off) f_off = min(f_off, key);
      if (bad) f_bad = min(f_bad, key);
      word = (on ? y * A.W + x : AUD_CID_OFF) | dir << AUD_CID_DIR_SHIFT | ((jump || off || bad) ? AUD_CID_VIOL : 0u);
    }
    s_cid[lane][a] = word;
    if (A.agent) {
      const uint32_t nm = (uint32_t)__popcll(__ballot(moved)), nd = (uint32_t)__popcll(__ballot(deliv));
      if (lane == 0) {
        if (nm) atomicAdd(&A.agent[(size_t)i * AUD_NAGENT + 0], nm);
        if (nd) atomicAdd(&A.agent[(size_t)i * AUD_NAGENT + 1], nd);
      }
    }
  }
  {
    const uint32_t cnt[AUD_A_NCNT] = {c_st0, c_st1, c_st2, c_st3, c_bad, c_moved, c_deliv, c_jump, c_off};
#pragma unroll
    for (uint32_t k = 0; k < AUD_A_NCNT; ++k)
      if (cnt[k]) atomicAdd(&s_cnt[lane][k], cnt[k]);
    if (f_jump != AUD_NONE) atomicMin(&s_first[0], f_jump);
    if (f_off != AUD_NONE) atomicMin(&s_first[1], f_off);
    if (f_bad != AUD_NONE) atomicMin(&s_first[2], f_bad);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < AUD_TILE_COLS * AUD_A_NCNT; k += AUD_A_BLOCK) {
    const uint32_t c = k / AUD_A_NCNT, j = k - c * AUD_A_NCNT;
    const uint32_t v = s_cnt[c][j];
    // counters 0-6 keep their place in a column's words; jumps and off_map sit behind pass B's two
    if (v && t0 + c < A.T) atomicAdd(&A.col[(size_t)(t0 + c) * AUD_NCOL + (j < 7u ? j : j + 2u)], v);
  }
  if (threadIdx.x < 3 && s_first[threadIdx.x] != AUD_NONE)
    atomicMin(&A.first[AUD_K_JUMP + threadIdx.x], s_first[threadIdx.x]);
  // the transpose: a wave writes one column of the tile, lane = agent
  for (uint32_t c = wave; c < AUD_TILE_COLS; c += AUD_A_WAVES) {
    const uint32_t tt = t0 + c, i = i0 + lane;
    if (tt < A.T && i < A.n) A.cid[(size_t)tt * A.n + i] = s_cid[c][lane];
  }
}

__device__ inline uint32_t aud_delta(uint32_t dir, uint32_t W) {  // cell - the cell left, two's complement
  return dir == AUD_DIR_E ? 1u : dir == AUD_DIR_W ? 0u - 1u : dir == AUD_DIR_S ? W : 0u - W;
}

// The entry under the tag of the current column: what it holds if it was written in this column, else empty.
__device__ inline unsigned long long aud_current(unsigned long long e, unsigned long long tag) {
  return (e >> AUD_E_TAG_SHIFT) == (tag >> AUD_E_TAG_SHIFT) ? e : tag | 0xFFFFFFFFull;
}

template <bool LDS>
__device__ inline unsigned long long aud_load(unsigned long long* p) {
  if (LDS) return *p;
  // the entry was written by atomics, which complete in L2: read it there, not from this CU's L1
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// entry.agent = min(entry.agent, i)
template <bool LDS>
__device__ inline void aud_occupy(unsigned long long* p, unsigned long long tag, uint32_t i) {
  unsigned long long old = aud_load<LDS>(p);
  for (;;) {
    const unsigned long long cur = aud_current(old, tag);
    if (cur == old && (uint32_t)cur <= i) return;
    const unsigned long long want = (uint32_t)cur <= i ? cur : (cur & ~0xFFFFFFFFull) | i;
    const unsigned long long seen = atomicCAS(p, old, want);
    if (seen == old) return;
    old = seen;
  }
}

// entry.dirs |= 1 << dir
template <bool LDS>
__device__ inline void aud_leave(unsigned long long* p, unsigned long long tag, uint32_t dir) {
  const unsigned long long bit = 1ull << (AUD_E_DIR_SHIFT + dir);
  unsigned long long old = aud_load<LDS>(p);
  for (;;) {
    const unsigned long long cur = aud_current(old, tag);
    if (cur == old && (cur & bit)) return;
    const unsigned long long seen = atomicCAS(p, old, cur | bit);
    if (seen == old) return;
    old = seen;
  }
}

template <bool LDS>
__global__ __launch_bounds__(AUD_B_BLOCK) void k_audit_columns(AuditArgs A) {
  extern __shared__ unsigned long long s_tab[];  // LDS: the table, W * H entries
  __shared__ uint32_t s_cnt[2][2];               // [column parity][colocations, swaps]
  __shared__ unsigned long long s_first[2];
  const uint32_t ncell = A.W * A.H;
  unsigned long long* tab = LDS ? s_tab : A.tab + (size_t)blockIdx.x * ncell;
  if (LDS)
    for (uint32_t c = threadIdx.x; c < ncell; c += AUD_B_BLOCK) s_tab[c] = 0;
  if (threadIdx.x < 4) (&s_cnt[0][0])[threadIdx.x] = 0;
  if (threadIdx.x < 2) s_first[threadIdx.x] = AUD_NONE;
  __syncthreads();

  unsigned long long f_coloc = AUD_NONE, f_swap = AUD_NONE;
  uint32_t k = 0;  // this workgroup's k-th column
  for (uint32_t t = blockIdx.x; t < A.T; t += A.G, ++k) {
    const unsigned long long tag = (unsigned long long)(k + 1u) << AUD_E_TAG_SHIFT;
    const uint32_t* cid = A.cid + (size_t)t * A.n;
    for (uint32_t i = threadIdx.x; i < A.n; i += AUD_B_BLOCK) {
      const uint32_t w = cid[i], c = w & AUD_CID_MASK, d = (w >> AUD_CID_DIR_SHIFT) & 7u;
      if (c >= ncell) continue;  // AUD_CID_OFF
      aud_occupy<LDS>(&tab[c], tag, i);
      if (d) {
        const uint32_t from = c - aud_delta(d - 1u, A.W);
        if (from < ncell) aud_leave<LDS>(&tab[from], tag, d - 1u);
      }
    }
    __syncthreads();
    uint32_t nco = 0, nsw = 0;
    for (uint32_t i = threadIdx.x; i < A.n; i += AUD_B_BLOCK) {
      const uint32_t w = cid[i], c = w & AUD_CID_MASK, d = (w >> AUD_CID_DIR_SHIFT) & 7u;
      bool coloc = false, swap = false;
      if (c < ncell) {
        const unsigned long long e = aud_load<LDS>(&tab[c]);
        coloc = (uint32_t)e != i;
        swap = d != 0 && ((e >> (AUD_E_DIR_SHIFT + ((d - 1u) ^ 1u))) & 1ull);
      }
      const unsigned long long key = (unsigned long long)t << 32 | i;
      if (coloc) {
        ++nco;
        f_coloc = min(f_coloc, key);
      }
      if (swap) {
        ++nsw;
        f_swap = min(f_swap, key);
      }
      if (A.agent && (coloc || swap || (w & AUD_CID_VIOL))) {
        atomicAdd(&A.agent[(size_t)i * AUD_NAGENT + 2], 1u);
        atomicMin(&A.agent[(size_t)i * AUD_NAGENT + 3], t);
      }
    }
    if (nco) atomicAdd(&s_cnt[k & 1u][0], nco);
    if (nsw) atomicAdd(&s_cnt[k & 1u][1], nsw);
    __syncthreads();  // phase 2 has read the table: the next column may write it
    if (threadIdx.x == 0) {  // this parity's counters are next added to two barriers from here
      A.col[(size_t)t * AUD_NCOL + AUD_C_COLOC] = s_cnt[k & 1u][0];
      A.col[(size_t)t * AUD_NCOL + AUD_C_SWAP] = s_cnt[k & 1u][1];
      s_cnt[k & 1u][0] = s_cnt[k & 1u][1] = 0;
    }
  }
  if (f_coloc != AUD_NONE) atomicMin(&s_first[0], f_coloc);
  if (f_swap != AUD_NONE) atomicMin(&s_first[1], f_swap);
  __syncthreads();
  if (threadIdx.x < 2 && s_first[threadIdx.x] != AUD_NONE)
    atomicMin(&A.first[AUD_K_COLOC + threadIdx.x], s_first[threadIdx.x]);
}

}  // namespace

size_t aud_lds_bytes(uint32_t ncell) { return (size_t)ncell * 8 + 64; }  // the table and the kernel's own words

bool aud_tab_in_lds(uint32_t ncell, int max_lds) { return max_lds > 0 && aud_lds_bytes(ncell) <= (size_t)max_lds; }

uint32_t aud_workgroups(uint32_t T, uint32_t ncell, bool in_lds) {
  size_t g = std::min<size_t>(T, AUD_G_MAX);
  if (!in_lds) g = std::min(g, AUD_TAB_BUDGET / ((size_t)std::max(ncell, 1u) * 8));
  return (uint32_t)std::max<size_t>(g, 1);
}

hipError_t launch_audit_rows(const AuditArgs& A, hipStream_t s) {
  if (A.n == 0 || A.T == 0) return hipSuccess;
  const dim3 grid((A.n + AUD_TILE_AGENTS - 1) / AUD_TILE_AGENTS, (A.T + AUD_TILE_COLS - 1) / AUD_TILE_COLS);
  hipLaunchKernelGGL(k_audit_rows, grid, dim3(AUD_A_BLOCK), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_audit_columns(const AuditArgs& A, int max_lds, hipStream_t s) {
  if (A.n == 0 || A.T == 0) return hipSuccess;
  if (A.G == 0 || A.G > AUD_G_MAX) return hipErrorInvalidValue;
  if (A.tab) {
    hipLaunchKernelGGL(k_audit_columns<false>, dim3(A.G), dim3(AUD_B_BLOCK), 0, s, A);
    return hipGetLastError();
  }
  const size_t lds = (size_t)A.W * A.H * 8;
  if (!aud_tab_in_lds(A.W * A.H, max_lds)) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute((const void*)k_audit_columns<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_audit_columns<true>, dim3(A.G), dim3(AUD_B_BLOCK), lds, s, A);
  return hipGetLastError();
}

}  // namespace tsw

// tsw_audit.h — host-callable launch wrappers for the kernels in tsw_audit.hip (K6: the audit of plan
// records, in the definitions above tsw_audit_records in include/tswap.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tsw {

// pass A works on tiles of AUD_TILE_AGENTS agents x AUD_TILE_COLS columns, one AUD_A_BLOCK-thread workgroup each
constexpr uint32_t AUD_TILE_AGENTS = 64u, AUD_TILE_COLS = 64u, AUD_A_BLOCK = 256u;
// pass B: columns strided over at most AUD_G_MAX workgroups of AUD_B_BLOCK threads
constexpr uint32_t AUD_G_MAX = 128u, AUD_B_BLOCK = 1024u;
// the occupancy tables of pass B outside LDS: at most this many bytes over all workgroups
constexpr size_t AUD_TAB_BUDGET = (size_t)256 << 20;

constexpr uint32_t AUD_NCOL = 11u, AUD_NAGENT = 4u, AUD_NKIND = 5u;  // TSW_AUDIT_* of include/tswap.h
// col[t * AUD_NCOL + k]
enum : uint32_t { AUD_C_STATE = 0, AUD_C_BAD = 4, AUD_C_MOVED = 5, AUD_C_DELIV = 6, AUD_C_COLOC = 7, AUD_C_SWAP = 8,
                  AUD_C_JUMP = 9, AUD_C_OFF = 10 };
// violation kinds, the order of tsw_audit::first_t
enum : uint32_t { AUD_K_COLOC = 0, AUD_K_SWAP = 1, AUD_K_JUMP = 2, AUD_K_OFF = 3, AUD_K_BAD = 4 };

// One word of the column-major transpose pass A hands to pass B (cid[t * n + i]):
//   bits 0-23  cell id, AUD_CID_OFF for a record off the grid (cells <= 2^20)
//   bits 24-26 0, or 1 + the direction of a unit step from column t - 1 with both records on the grid
//              (AUD_DIR_*): the cell left is then cell - aud_delta(direction, W)
//   bit 31     the record is charged with a jump, an off_map or a bad_state (pass A's kinds)
constexpr uint32_t AUD_CID_MASK = 0xFFFFFFu, AUD_CID_OFF = 0xFFFFFFu, AUD_CID_DIR_SHIFT = 24u, AUD_CID_VIOL = 1u << 31;
enum : uint32_t { AUD_DIR_E = 0, AUD_DIR_W = 1, AUD_DIR_S = 2, AUD_DIR_N = 3 };  // the reverse is direction ^ 1

// One entry of pass B's occupancy table, per cell: the column tag of the owning workgroup (its k-th column
// has tag k + 1; 0 = never written, so the table is cleared once per call and never between columns), the
// directions in which agents leave the cell in the transition into the column, and the smallest agent
// index on the cell in the column.
constexpr uint32_t AUD_E_TAG_SHIFT = 36u, AUD_E_DIR_SHIFT = 32u;

struct AuditArgs {
  uint32_t n, T, W, H, Ww;
  size_t stride;                  // records per agent row
  const unsigned long long* rec;  // tsw_rec as x | y << 16 | state << 32 | pad << 40, agent-major
  const uint32_t* freebits;       // DevGrid::freebits
  uint32_t* cid;                  // [T * n] the column-major transpose, words as above
  uint32_t* col;                  // [T * AUD_NCOL], zero before pass A
  uint32_t* agent;                // [n * AUD_NAGENT] or nullptr; moves, deliveries, columns = 0 and first = ~0 before pass A
  unsigned long long* first;      // [AUD_NKIND] t << 32 | agent of the first violation per kind, ~0 before pass A
  unsigned long long* tab;        // pass B outside LDS: G * W * H entries, zero; nullptr: the table lives in LDS
  uint32_t G;                     // workgroups of pass B
};

// bytes of LDS pass B needs with the table inside (aud_tab_in_lds: it fits a workgroup's limit)
size_t aud_lds_bytes(uint32_t ncell);
bool aud_tab_in_lds(uint32_t ncell, int max_lds);
// workgroups of pass B for T columns on ncell cells (>= 1)
uint32_t aud_workgroups(uint32_t T, uint32_t ncell, bool in_lds);

hipError_t launch_audit_rows(const AuditArgs& A, hipStream_t s);                  // pass A
hipError_t launch_audit_columns(const AuditArgs& A, int max_lds, hipStream_t s);  // pass B

}  // namespace tsw

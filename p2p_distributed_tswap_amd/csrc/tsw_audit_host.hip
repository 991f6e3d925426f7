// tsw_audit_host.hip — the audit of plan records in the host runtime (tsw_ctx.h): tsw_audit_records and
// tsw_audit_records_device around the two passes of K6 (tsw_audit.hip). The call reads the context's grid
// and nothing else of it: the table store, the queues and the stats stay as they were. Host code only.
#include "tsw_audit.h"
#include "tsw_ctx.h"
#include "tsw_layout.h"

namespace tsw {

int upload_records(tsw_ctx* c, const tsw_rec* rec, uint32_t n, uint32_t T, uint32_t stride, const char* label) {
  TRY(scratch_grow(c, c->d_aud_rec, (size_t)n * T, label, "records"));
  if (stride == T)
    HIPCHK(hipMemcpyAsync(c->d_aud_rec, rec, (size_t)n * T * 8, hipMemcpyHostToDevice, c->s));
  else
    HIPCHK(hipMemcpy2DAsync(c->d_aud_rec, (size_t)T * 8, rec, (size_t)stride * 8, (size_t)T * 8, n, hipMemcpyHostToDevice, c->s));
  return TSW_OK;
}

}  // namespace tsw

extern "C" {

static void audit_empty(tsw_audit* sum) {
  std::memset(sum, 0, sizeof *sum);
  for (uint32_t k = 0; k < TSW_AUDIT_NKIND; ++k) sum->first_t[k] = sum->first_agent[k] = 0xFFFFFFFFu;
}

// d_rec: the records on the device, agent-major with `stride` records per row
static int audit_device(tsw_ctx* c, const unsigned long long* d_rec, uint32_t n, uint32_t T, size_t stride,
                        tsw_audit* sum, uint32_t* col, uint32_t* agent) {
  const uint32_t ncell = c->G.ncell;
  const bool in_lds = aud_tab_in_lds(ncell, c->max_lds);
  AuditArgs A{};
  A.n = n;
  A.T = T;
  A.W = c->G.W;
  A.H = c->G.H;
  A.Ww = c->G.Ww;
  A.stride = stride;
  A.rec = d_rec;
  A.freebits = c->G.freebits;
  A.G = aud_workgroups(T, ncell, in_lds);
  const AuditOutLayout L = audit_out_layout(n, T, agent != nullptr, AUD_NKIND, AUD_NCOL, AUD_NAGENT);
  TRY(scratch_grow(c, c->d_aud_out, L.total, "audit", "counters"));
  TRY(scratch_grow(c, c->d_aud_cid, (size_t)T * n, "audit", "transpose"));
  if (!in_lds) TRY(scratch_grow(c, c->d_aud_tab, (size_t)A.G * ncell, "audit", "occupancy tables"));
  uint32_t* const d = c->d_aud_out.p;
  A.first = reinterpret_cast<unsigned long long*>(d + L.first);
  A.col = d + L.col;
  A.agent = agent ? d + L.agent : nullptr;
  A.cid = c->d_aud_cid;
  A.tab = in_lds ? nullptr : c->d_aud_tab.p;
  HIPCHK(hipMemsetAsync(A.first, 0xFF, AUD_NKIND * 8, c->s));
  HIPCHK(hipMemsetAsync(A.col, 0, L.col_words * 4, c->s));
  if (agent) {  // moves, deliveries, columns = 0; first = 0xFFFFFFFF
    HIPCHK(hipMemsetAsync(A.agent, 0, L.agent_words * 4, c->s));
    HIPCHK(hipMemset2DAsync(A.agent + 3, AUD_NAGENT * 4, 0xFF, 4, n, c->s));
  }
  if (!in_lds) HIPCHK(hipMemsetAsync(A.tab, 0, (size_t)A.G * ncell * 8, c->s));
  HIPCHK(launch_audit_rows(A, c->s));
  HIPCHK(launch_audit_columns(A, c->max_lds, c->s));
  // first | col come down together; the sums are the host's (T * AUD_NCOL additions)
  std::vector<uint32_t> h(L.col + L.col_words);
  HIPCHK(hipMemcpyAsync(h.data(), d + L.first, h.size() * 4, hipMemcpyDeviceToHost, c->s));
  if (agent) HIPCHK(hipMemcpyAsync(agent, A.agent, L.agent_words * 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  const uint32_t* hc = h.data() + L.col;
  audit_empty(sum);
  for (uint32_t t = 0; t < T; ++t) {
    const uint32_t* w = hc + (size_t)t * AUD_NCOL;
    for (uint32_t k = 0; k < 4; ++k) sum->state_steps[k] += w[AUD_C_STATE + k];
    sum->bad_state += w[AUD_C_BAD];
    sum->moves += w[AUD_C_MOVED];
    sum->deliveries += w[AUD_C_DELIV];
    sum->colocations += w[AUD_C_COLOC];
    sum->swaps += w[AUD_C_SWAP];
    sum->jumps += w[AUD_C_JUMP];
    sum->off_map += w[AUD_C_OFF];
    if (t > 0 && w[AUD_C_MOVED]) ++sum->moving_columns;
  }
  for (uint32_t k = 0; k < AUD_NKIND; ++k) {
    unsigned long long key;
    std::memcpy(&key, h.data() + L.first + 2 * k, 8);
    if (key != ~0ull) {
      sum->first_t[k] = (uint32_t)(key >> 32);
      sum->first_agent[k] = (uint32_t)key;
    }
  }
  if (col) std::memcpy(col, hc, L.col_words * 4);
  return TSW_OK;
}

// what both entry points check before anything is launched; *empty: nothing to audit, *sum is final
static int audit_check(tsw_ctx* c, const tsw_rec* rec, uint32_t n, uint32_t T, uint32_t stride, tsw_audit* sum,
                       bool* empty) {
  NOT_FROM_RESOLVER(c);
  if (!sum) RET(TSW_EINVAL, "null sum");
  if (!rec && n > 0 && T > 0) RET(TSW_EINVAL, "null rec");
  if (stride < T) RET(TSW_EINVAL, "stride is smaller than T");
  if (T > (1u << 20) + 1u) RET(TSW_EINVAL, "T too large");
  *empty = n == 0 || T == 0;
  if (*empty) audit_empty(sum);
  return TSW_OK;
}

int tsw_audit_records_device(tsw_ctx* c, const tsw_rec* dev_rec, uint32_t n, uint32_t T, uint32_t stride,
                             tsw_audit* sum, uint32_t* col, uint32_t* agent) {
  if (!c) return TSW_EINVAL;
  bool empty = false;
  TRY(audit_check(c, dev_rec, n, T, stride, sum, &empty));
  if (empty) return TSW_OK;
  TRY(set_device(c));
  HIPCHK(hipDeviceSynchronize());  // dev_rec may have been produced on another stream of the caller
  return audit_device(c, reinterpret_cast<const unsigned long long*>(dev_rec), n, T, stride, sum, col, agent);
}

int tsw_audit_records(tsw_ctx* c, const tsw_rec* rec, uint32_t n, uint32_t T, uint32_t stride, tsw_audit* sum,
                      uint32_t* col, uint32_t* agent) {
  if (!c) return TSW_EINVAL;
  bool empty = false;
  TRY(audit_check(c, rec, n, T, stride, sum, &empty));
  if (empty) return TSW_OK;
  TRY(set_device(c));
  // columns 0 .. T - 1 of every row go up, packed: the device copy has T records per row
  TRY(upload_records(c, rec, n, T, stride, "audit"));
  return audit_device(c, c->d_aud_rec, n, T, T, sum, col, agent);
}

}  // extern "C"

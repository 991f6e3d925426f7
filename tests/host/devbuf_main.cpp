// Stand-alone check of csrc/tsw_buf.h (DevBuf / PinnedBuf) under ASan + UBSan, with no HIP library and no
// device: this file supplies the five HIP allocation calls itself, backed by malloc. The fakes count the
// live blocks and can be told to fail the k-th allocation from now. Exits non-zero on any mismatch, or
// when a block is still live at the end; a double free or a use after free is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "../../p2p_distributed_tswap_amd/csrc/tsw_buf.h"

namespace {

std::set<void*> g_dev, g_host;  // live blocks
long g_fail_in = 0;             // > 0: the g_fail_in-th allocation from now fails
int g_frees = 0;
int g_bad = 0;

bool fail_now() { return g_fail_in > 0 && --g_fail_in == 0; }
size_t live() { return g_dev.size() + g_host.size(); }

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);    \
      ++g_bad;                                                        \
    }                                                                 \
  } while (0)

}  // namespace

extern "C" {

hipError_t hipMalloc(void** p, size_t bytes) {
  if (fail_now()) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);
  g_dev.insert(*p);
  return hipSuccess;
}

hipError_t hipFree(void* p) {
  if (!g_dev.erase(p)) {
    std::printf("hipFree of a block that is not live\n");
    ++g_bad;
    return hipErrorInvalidValue;
  }
  ++g_frees;
  std::free(p);
  return hipSuccess;
}

hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
  if (fail_now()) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);
  g_host.insert(*p);
  return hipSuccess;
}

hipError_t hipHostFree(void* p) {
  if (!g_host.erase(p)) {
    std::printf("hipHostFree of a block that is not live\n");
    ++g_bad;
    return hipErrorInvalidValue;
  }
  ++g_frees;
  std::free(p);
  return hipSuccess;
}

// the fake device sees host memory at its own address
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) {
  if (!g_host.count(host)) return hipErrorInvalidValue;
  *dev = host;
  return hipSuccess;
}

}  // extern "C"

using tsw::DevBuf;
using tsw::PinnedBuf;

static void growth() {
  DevBuf<uint32_t> b;
  CHECK(!b.p && b.cap == 0 && !b.holds(0));
  CHECK(b.grow(5) == hipSuccess);  // from empty: max(5, max(0, 16))
  CHECK(b.p && b.cap == 16 && live() == 1);
  b.p[15] = 7;  // the whole capacity is the block's
  uint32_t* p0 = b.p;
  CHECK(b.grow(16) == hipSuccess && b.p == p0 && b.cap == 16);  // within capacity: the pointer stays
  CHECK(b.grow(0) == hipSuccess && b.p == p0);
  CHECK(b.grow(17) == hipSuccess && b.cap == 24 && live() == 1);  // max(17, 16 + 8)
  CHECK(b.grow(100) == hipSuccess && b.cap == 100 && live() == 1);  // max(100, 36)
  CHECK(b.grow(101) == hipSuccess && b.cap == 150);                 // max(101, 150)
  b.p[149] = 1;
  CHECK(b.alloc(3) == hipSuccess && b.cap == 3 && live() == 1);  // exact, also downwards
  CHECK(b.reset() == hipSuccess && !b.p && b.cap == 0 && live() == 0);
  CHECK(b.reset() == hipSuccess);  // empty: nothing to free
}

static void failures() {
  DevBuf<uint64_t> b;
  CHECK(b.grow(40) == hipSuccess && b.cap == 40);
  int f0 = g_frees;
  g_fail_in = 1;
  CHECK(b.grow(41) == hipErrorOutOfMemory);
  CHECK(!b.p && b.cap == 0 && live() == 0 && g_frees == f0 + 1);  // the old block went exactly once
  CHECK(b.grow(41) == hipSuccess && b.cap == 41 && live() == 1);  // max(41, 16): the capacity restarted at 0
  f0 = g_frees;
  g_fail_in = 1;
  CHECK(b.alloc(8) == hipErrorOutOfMemory && !b.p && b.cap == 0 && live() == 0 && g_frees == f0 + 1);
  g_fail_in = 1;
  CHECK(b.alloc(8) == hipErrorOutOfMemory && g_frees == f0 + 1);  // empty and failing: nothing to free
  CHECK(b.alloc(8) == hipSuccess && b.cap == 8);
  b.p[7] = 1;
}

static void moves() {
  DevBuf<uint8_t> a;
  CHECK(a.alloc(10) == hipSuccess);
  uint8_t* p = a.p;
  DevBuf<uint8_t> b(std::move(a));
  CHECK(!a.p && a.cap == 0 && b.p == p && b.cap == 10 && live() == 1);
  DevBuf<uint8_t> c;
  CHECK(c.alloc(4) == hipSuccess && live() == 2);
  c = std::move(b);  // frees c's own block, takes b's
  CHECK(!b.p && b.cap == 0 && c.p == p && c.cap == 10 && live() == 1);
  DevBuf<uint8_t>& self = c;
  c = std::move(self);
  CHECK(c.p == p && c.cap == 10 && live() == 1);
  PinnedBuf<uint32_t> h;
  CHECK(h.alloc(6, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess && h.map() == hipSuccess);
  PinnedBuf<uint32_t> h2(std::move(h));
  CHECK(!h.p && !h.dev && h.cap == 0 && h2.p && h2.dev == h2.p && h2.cap == 6);
  PinnedBuf<uint32_t> h3;
  h3 = std::move(h2);
  CHECK(!h2.p && !h2.dev && h2.cap == 0 && h3.dev == h3.p && h3.cap == 6 && live() == 2);
}

// ensure_agents' shape: thirteen arrays allocated in sequence, the allocation failing at each position in turn
static void thirteen() {
  for (int fail = 1; fail <= 13; ++fail) {
    {
      DevBuf<uint32_t> arr[13];
      for (auto& b : arr) CHECK(b.alloc(64) == hipSuccess);  // the arrays of an earlier, smaller fleet
      CHECK(live() == 13);
      g_fail_in = fail;
      int done = 0;
      for (; done < 13; ++done)
        if (arr[done].alloc(128) != hipSuccess) break;
      CHECK(done == fail - 1);
      for (int i = 0; i < 13; ++i) {  // every member is whole or empty
        const size_t want = i < done ? 128u : i == done ? 0u : 64u;
        CHECK(arr[i].cap == want && (arr[i].p != nullptr) == (want != 0));
        if (arr[i].p) arr[i].p[want - 1] = 1;
      }
      CHECK(live() == 12);
    }
    CHECK(live() == 0);  // destruction frees what is left, once
  }
  g_fail_in = 0;
}

static void pinned() {
  PinnedBuf<uint32_t> plain, mapped;
  CHECK(plain.alloc(1) == hipSuccess && plain.p && !plain.dev && plain.cap == 1 && plain.holds(1));
  *plain = 5;
  CHECK(mapped.alloc(64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess && !mapped.dev);
  CHECK(mapped.map() == hipSuccess && mapped.dev == mapped.p && mapped.cap == 64);
  mapped.dev[63] = 9;
  CHECK(mapped.p[63] == 9 && live() == 2);
  CHECK(mapped.alloc(128) == hipSuccess && !mapped.dev && mapped.cap == 128 && live() == 2);  // the alias went with the block
  g_fail_in = 1;
  CHECK(mapped.alloc(256) == hipErrorOutOfMemory && !mapped.p && !mapped.dev && mapped.cap == 0 && live() == 1);
  CHECK(mapped.alloc(2) == hipSuccess && mapped.cap == 2);
  CHECK(plain.reset() == hipSuccess && !plain.p && live() == 1);
}

int main() {
  growth();
  failures();
  CHECK(live() == 0);
  moves();
  CHECK(live() == 0);
  thirteen();
  pinned();
  if (live() != 0) {
    std::printf("%zu block(s) still live at exit\n", live());
    return 1;
  }
  if (g_bad) return 1;
  std::printf("devbuf sanitizer run ok\n");
  return 0;
}

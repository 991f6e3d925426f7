// Stand-alone driver for the host A* request ring's match test (csrc/tsw_plan.h: host_req_word,
// host_req_live, host_reply_match), built with the host compiler alone — no HIP, no device — under
// ASan + UBSan by tests/test_host_ask_match.py. Exits non-zero on the first failed case.
#include <cstdint>
#include <cstdio>

#include "tsw_plan.h"

using namespace tsw;

static int fails = 0;

static void expect(const char* name, bool got, bool want) {
  if (got != want) {
    std::printf("FAIL %s: got %d want %d\n", name, (int)got, (int)want);
    ++fails;
  } else {
    std::printf("ok   %s\n", name);
  }
}

static uint32_t reply(uint32_t ticket, uint32_t code) { return ((ticket + 1u) << 8) | code; }

int main() {
  const uint32_t v = 1234u, g = 4321u;
  uint8_t code = 0xEEu;

  // an exact match: ticket 5 of 9 taken, ring of 16, code 2
  {
    const unsigned long long w = host_req_word(5u, v, g);
    code = 0xEEu;
    expect("exact match", host_reply_match(w, reply(5u, 2u), v, g, 9u, 16u, &code), true);
    expect("exact match: code", code == 2u, true);
    uint32_t t = ~0u;
    expect("exact match: live", host_req_live(w, v, g, 9u, 16u, &t), true);
    expect("exact match: ticket", t == 5u, true);
    // every code up to NH_STAY counts
    for (uint32_t c = 0; c <= NH_STAY; ++c) {
      code = 0xEEu;
      expect("codes 0..4", host_reply_match(w, reply(5u, c), v, g, 9u, 16u, &code) && code == c, true);
    }
  }

  // a zeroed ring: no remembered word, no reply word; and a request without a reply yet
  {
    code = 0xEEu;
    expect("zeroed slot, zeroed reply", host_reply_match(0ull, 0u, v, g, 9u, 16u, &code), false);
    expect("zeroed slot, zeroed reply, pair (0, 0), no ticket taken", host_reply_match(0ull, 0u, 0u, 0u, 0u, 16u, &code), false);
    expect("zeroed slot, pair (0, 0)", host_reply_match(0ull, reply(0u, 1u), 0u, 0u, 1u, 16u, &code), false);
    expect("zeroed slot is not live", host_req_live(0ull, 0u, 0u, 9u, 16u), false);
    expect("request without a reply", host_reply_match(host_req_word(0u, v, g), 0u, v, g, 1u, 16u, &code), false);
    expect("code untouched on a mismatch", code == 0xEEu, true);
  }

  // the same slot after a wrap: ring of 8, ticket t against t + 8 (both map to slot t % 8)
  {
    const uint32_t t = 3u;
    const unsigned long long w = host_req_word(t, v, g);
    // ticket t + 8 not taken yet, its reply cannot be there; once taken and answered the slot carries seq t + 9
    expect("wrap: reply of t + 8 against the word of t", host_reply_match(w, reply(t + 8u, 1u), v, g, t + 9u, 8u, &code), false);
    expect("wrap: reply of t + 8, window still open", host_reply_match(w, reply(t + 8u, 1u), v, g, t + 8u, 8u, &code), false);
    expect("wrap: the word of t + 8 takes it", host_reply_match(host_req_word(t + 8u, v, g), reply(t + 8u, 1u), v, g, t + 9u, 8u, &code), true);
    expect("wrap: reply of t against the word of t + 8", host_reply_match(host_req_word(t + 8u, v, g), reply(t, 1u), v, g, t + 9u, 8u, &code), false);
  }

  // a ticket outside the window: ring of 8, ticket 3; the slot is ticket 11's once 12 tickets are taken
  {
    const unsigned long long w = host_req_word(3u, v, g);
    expect("window: 11 tickets taken (last one inside)", host_reply_match(w, reply(3u, 0u), v, g, 11u, 8u, &code), true);
    expect("window: 12 tickets taken (outside)", host_reply_match(w, reply(3u, 0u), v, g, 12u, 8u, &code), false);
    expect("window: live at 11", host_req_live(w, v, g, 11u, 8u), true);
    expect("window: not live at 12", host_req_live(w, v, g, 12u, 8u), false);
    expect("window: a ticket not taken yet", host_req_live(w, v, g, 3u, 8u), false);
  }

  // another pair under the same ticket
  {
    const unsigned long long w = host_req_word(5u, v, g);
    expect("other start cell", host_reply_match(w, reply(5u, 2u), v + 1u, g, 9u, 16u, &code), false);
    expect("other goal", host_reply_match(w, reply(5u, 2u), v, g + 1u, 9u, 16u, &code), false);
    expect("start and goal exchanged", host_reply_match(w, reply(5u, 2u), g, v, 9u, 16u, &code), false);
  }

  // a code of 5 (> NH_STAY), and the unresolved marks
  {
    const unsigned long long w = host_req_word(5u, v, g);
    code = 0xEEu;
    expect("code 5", host_reply_match(w, reply(5u, 5u), v, g, 9u, 16u, &code), false);
    expect("code NH_UNKNOWN", host_reply_match(w, reply(5u, NH_UNKNOWN), v, g, 9u, 16u, &code), false);
    expect("code NH_PENDING", host_reply_match(w, reply(5u, NH_PENDING), v, g, 9u, 16u, &code), false);
    expect("code untouched", code == 0xEEu, true);
  }

  // the largest ticket: tickets stay below HOST_RING_MAX_TICKETS, so the last one has seq == HOST_RING_MAX_TICKETS
  {
    const uint32_t t = HOST_RING_MAX_TICKETS - 1u, ring = 1u << 14;
    const unsigned long long w = host_req_word(t, v, g);
    code = 0xEEu;
    expect("largest ticket: seq fits 24 bits", (uint32_t)(w >> 40) == HOST_RING_MAX_TICKETS && (reply(t, 3u) >> 8) == HOST_RING_MAX_TICKETS, true);
    expect("largest ticket", host_reply_match(w, reply(t, 3u), v, g, HOST_RING_MAX_TICKETS, ring, &code) && code == 3u, true);
    expect("largest ticket: the reply before it", host_reply_match(w, reply(t - ring, 3u), v, g, HOST_RING_MAX_TICKETS, ring, &code), false);
    expect("past the largest ticket", host_req_live(host_req_word(HOST_RING_MAX_TICKETS, v, g), v, g, HOST_RING_MAX_TICKETS + 1u, ring), false);
  }

  // cells at 2^20 - 1: the fields do not run into each other or into the seq
  {
    const uint32_t big = (1u << 20) - 1u;
    const unsigned long long w = host_req_word(7u, big, big);
    code = 0xEEu;
    expect("cells 2^20 - 1: layout", (uint32_t)(w >> 40) == 8u && ((uint32_t)(w >> 20) & 0xFFFFFu) == big && ((uint32_t)w & 0xFFFFFu) == big, true);
    expect("cells 2^20 - 1", host_reply_match(w, reply(7u, 4u), big, big, 8u, 16u, &code) && code == 4u, true);
    expect("cells 2^20 - 1 against (2^20 - 1, 0)", host_reply_match(w, reply(7u, 4u), big, 0u, 8u, 16u, &code), false);
    expect("cells 2^20 - 1 against (0, 2^20 - 1)", host_reply_match(w, reply(7u, 4u), 0u, big, 8u, 16u, &code), false);
    expect("(2^20 - 1, 0) against (2^20 - 2, 2^20 - 1)", host_reply_match(host_req_word(7u, big, 0u), reply(7u, 4u), big - 1u, big, 8u, 16u, &code), false);
  }

  if (fails) {
    std::printf("%d case(s) failed\n", fails);
    return 1;
  }
  std::printf("host ask match ok\n");
  return 0;
}

// row_declines.cpp -- a query's decline mask (csrc/mrk_host_int.h: row_decline_mask), host only, under AddressSanitizer + UBSan: one bit
// per exchange-row format (ROWS_NARROW, ROWS_WIDE, ROWS_ORDER), set when the query's row of that format leaves the batch empty with
// MRK_ROW_DECLINED.  Every combination of status {MRK_OK, MRK_E_UNSUPPORTED} x order {0, SORT_ON_ATTR, SORT_ON_ORDER, SORT_ON_WEIGHT}
// x sort bits {0, 17} x the weight-first switch {0, 1} against a table written out below from the rule
//   narrow: status != MRK_OK || bits != 0 || order == SORT_ON_ORDER || order == SORT_ON_WEIGHT
//   wide:   status != MRK_OK || order == SORT_ON_ORDER || order == SORT_ON_WEIGHT
//   order:  status != MRK_OK || (order == SORT_ON_WEIGHT && !switch)
// and the property the batch relied on while it kept the order rows' words in a plane of their own, uploaded only with a submit that
// held a SORT_ON_ORDER query or, under the switch, a SORT_ON_WEIGHT one: in every other submit the order bit equals the wide bit for
// every query.  Built and run by tests/test_row_declines_cpu.py; no GPU, no libmrk.so.
#include <stdint.h>
#include <stdio.h>

#include "../../manticoresearch_amd/csrc/mrk_host_int.h"

static int g_bad = 0;
#define CHECK(c, ...)                               \
  do {                                              \
    if (!(c)) {                                     \
      if (g_bad < 20) {                             \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                        \
        printf("\n");                               \
      }                                             \
      ++g_bad;                                      \
    }                                               \
  } while (0)

constexpr uint32_t N = 1, W = 2, O = 4; // the bits, as the kernels read them: 1 << ROWS_NARROW, 1 << ROWS_WIDE, 1 << ROWS_ORDER
static_assert(N == 1u << mrk::ROWS_NARROW && W == 1u << mrk::ROWS_WIDE && O == 1u << mrk::ROWS_ORDER, "one bit per row kind");
static_assert(mrk::SORT_ON_ATTR == 1 && mrk::SORT_ON_ORDER == 2 && mrk::SORT_ON_WEIGHT == 3, "the table's order axis");

// EXPECT[status][order][bits][switch]: status 0 = MRK_OK, 1 = MRK_E_UNSUPPORTED; order 0, SORT_ON_ATTR, SORT_ON_ORDER, SORT_ON_WEIGHT;
// bits 0 = 0, 1 = 17; switch off, on
static const uint32_t EXPECT[2][4][2][2] = {
    {
        // MRK_OK
        {{0, 0}, {N, N}},                 // a relevance query; a mrk_query.sort (order 0, bits 17): no narrow row
        {{0, 0}, {N, N}},                 // a one-part order: planned as a sort (bits 0 does not occur; the rule holds all the same)
        {{N | W, N | W}, {N | W, N | W}}, // a 64-bit key: order rows only
        {{N | W | O, N | W}, {N | W | O, N | W}}, // the weight in front: order rows, and only under the switch
    },
    {
        // MRK_E_UNSUPPORTED: every row, whatever else
        {{N | W | O, N | W | O}, {N | W | O, N | W | O}},
        {{N | W | O, N | W | O}, {N | W | O, N | W | O}},
        {{N | W | O, N | W | O}, {N | W | O, N | W | O}},
        {{N | W | O, N | W | O}, {N | W | O, N | W | O}},
    },
};

int main() {
  const int status[2] = {MRK_OK, MRK_E_UNSUPPORTED};
  const uint32_t order[4] = {0u, mrk::SORT_ON_ATTR, mrk::SORT_ON_ORDER, mrk::SORT_ON_WEIGHT}, bits[2] = {0u, 17u};
  unsigned checked = 0;
  for (int s = 0; s < 2; ++s)
    for (int o = 0; o < 4; ++o)
      for (int b = 0; b < 2; ++b)
        for (int w = 0; w < 2; ++w) {
          const uint32_t got = mrk::row_decline_mask(status[s], bits[b], order[o], w != 0);
          CHECK(got == EXPECT[s][o][b][w], "status %d order %u bits %u switch %d: mask %u, the rule says %u", status[s], order[o], bits[b], w, got, EXPECT[s][o][b][w]);
          CHECK(!(got & ~(N | W | O)), "no other bit");
          // some bit is set exactly when the narrow bit is: what any_declined may be computed from
          CHECK((got != 0) == ((got & N) != 0), "status %d order %u bits %u switch %d: a bit without the narrow bit", status[s], order[o], bits[b], w);
          // a submit "without an order plane": this query is neither SORT_ON_ORDER nor, under the switch, SORT_ON_WEIGHT -- and, as every
          // query of such a submit is so, the property is one of each query: the order bit equals the wide bit
          const bool plane = order[o] == mrk::SORT_ON_ORDER || (order[o] == mrk::SORT_ON_WEIGHT && w);
          if (!plane) CHECK(((got & O) != 0) == ((got & W) != 0), "status %d order %u bits %u switch %d: order bit != wide bit", status[s], order[o], bits[b], w);
          ++checked;
        }
  if (g_bad) {
    printf("%d failures\n", g_bad);
    return 1;
  }
  printf("ok row declines %u combinations\n", checked);
  return 0;
}

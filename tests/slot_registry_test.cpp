// Stand-alone check of the slot registry (csrc/slots.h): host logic only.
// Built and run by tests/test_slot_registry.py; exits non-zero at the first
// failed expectation.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "slots.h"

using srhip::SlotRegistry;
using Keys = std::vector<std::string>;

static int g_line = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);           \
      g_line = __LINE__;                                                \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static bool distinct_below(const std::vector<int>& s, int n) {
  std::set<int> seen;
  for (int v : s) {
    if (v < 0 || v >= n || !seen.insert(v).second) return false;
  }
  return true;
}

int main() {
  std::vector<int> a, b, c;
  {  // assignment: lowest free slots first, a held key keeps its slot
    SlotRegistry r(8);
    EXPECT(r.nslot() == 8);
    EXPECT(r.assign(Keys{"k0", "k1", "k2"}, 255, &a));
    EXPECT((a == std::vector<int>{0, 1, 2}));
    EXPECT(r.assign(Keys{"k2", "k9", "k0"}, 255, &b));
    EXPECT((b == std::vector<int>{2, 3, 0}));
    EXPECT(r.key(3) == "k9" && r.key(1) == "k1" && r.key(7).empty() && r.key(-1).empty() && r.key(8).empty());
    EXPECT(r.assign(Keys{}, 255, &c) && c.empty());
  }
  {  // more keys than slots: refused, nothing changed
    SlotRegistry r(2);
    EXPECT(r.assign(Keys{"a", "b"}, 255, &a));
    EXPECT(!r.assign(Keys{"c", "d", "e"}, 255, &b));
    EXPECT(r.key(0) == "a" && r.key(1) == "b");
    EXPECT(!r.assign(Keys{"a", "b"}, 1, &b));  // the limit counts as the slot count
    SlotRegistry none(0);
    EXPECT(!none.assign(Keys{"a"}, 255, &b));
    EXPECT(none.assign(Keys{}, 255, &b));
  }
  {  // least recently used goes first; slots of the program being assigned are skipped
    SlotRegistry r(4);
    EXPECT(r.assign(Keys{"a", "b"}, 255, &a));  // a:0 b:1   (clock 1)
    EXPECT(r.assign(Keys{"c", "d"}, 255, &a));  // c:2 d:3   (clock 2)
    EXPECT(r.assign(Keys{"a"}, 255, &a));       // a touched (clock 3): b is now the oldest
    EXPECT(r.assign(Keys{"e"}, 255, &a));
    EXPECT(a[0] == 1 && r.key(1) == "e");       // displaced b
    // c and d are the oldest now, but the program uses c itself: x takes d's slot, y the next oldest (a)
    EXPECT(r.assign(Keys{"x", "c", "y"}, 255, &a));
    EXPECT(a[1] == 2);
    EXPECT(a[0] == 3 && a[2] == 0);
    EXPECT(distinct_below(a, 4));
    EXPECT(r.key(1) == "e");
    // a displaced key comes back under whatever slot is free or oldest, never one of its own program
    EXPECT(r.assign(Keys{"b", "e"}, 255, &a));
    EXPECT(a[1] == 1 && a[0] != 1 && distinct_below(a, 4));
  }
  {  // a full turn-over: B displaces all of A, A again displaces all of B, slots stay distinct
    SlotRegistry r(3);
    EXPECT(r.assign(Keys{"a0", "a1", "a2"}, 255, &a));
    EXPECT(r.assign(Keys{"b0", "b1", "b2"}, 255, &b));
    EXPECT(distinct_below(b, 3));
    EXPECT(r.assign(Keys{"a0", "a1", "a2"}, 255, &c));
    EXPECT(distinct_below(c, 3));
    for (int k = 0; k < 3; ++k) EXPECT(r.key(c[(size_t)k]) == "a" + std::to_string(k));
  }
  {  // the limit: slots below it only; a key held at or above it moves down
    SlotRegistry r(8);
    EXPECT(r.assign(Keys{"p", "q", "r", "s", "t"}, 255, &a));  // 0..4
    EXPECT(r.assign(Keys{"t", "u"}, 3, &b));
    EXPECT(distinct_below(b, 3));
    EXPECT(r.key(4).empty());  // t left its old slot
    EXPECT(r.key(b[0]) == "t" && r.key(b[1]) == "u");
    // every key maps to one slot and every slot's key maps back
    EXPECT(r.assign(Keys{"p", "q", "r", "s", "t", "u"}, 255, &c));
    EXPECT(distinct_below(c, 8));
  }
  {  // many rounds against a model: assignments are always distinct, in range, and stable for held keys
    SlotRegistry r(6);
    unsigned x = 12345;
    std::vector<std::string> held(6);
    for (int round = 0; round < 2000; ++round) {
      Keys ks;
      std::set<int> ids;
      x = x * 1664525u + 1013904223u;
      const int n = 1 + (int)((x >> 16) % 6);
      while ((int)ids.size() < n) {
        x = x * 1664525u + 1013904223u;
        ids.insert((int)((x >> 16) % 14));
      }
      for (int id : ids) ks.push_back("key" + std::to_string(id));
      std::vector<std::string> before(6);
      for (int s = 0; s < 6; ++s) before[(size_t)s] = r.key(s);
      EXPECT(r.assign(ks, 255, &a));
      EXPECT(distinct_below(a, 6));
      for (size_t k = 0; k < ks.size(); ++k) {
        EXPECT(r.key(a[k]) == ks[k]);
        for (int s = 0; s < 6; ++s)
          if (before[(size_t)s] == ks[k]) EXPECT(a[k] == s);  // a held key kept its slot
      }
      std::set<std::string> names;
      for (int s = 0; s < 6; ++s)
        if (!r.key(s).empty()) EXPECT(names.insert(r.key(s)).second);  // no key in two slots
    }
  }
  std::printf("slot registry ok\n");
  return 0;
}

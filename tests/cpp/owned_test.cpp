// owned_test.cpp — csrc/owned.hpp alone, under plain g++ with AddressSanitizer + UBSan (tests/test_host_parsers_sanitized.py):
// int handles and a Release that counts, so every release is seen, with the handle it was given.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

#include "owned.hpp"

static std::vector<int> g_released;  // every handle Release was called with, in order
struct CountingRelease {
  int operator()(int h) const {
    g_released.push_back(h);
    return 7;  // (ignored by the owner)
  }
};
using Own = axw::Owned<int, CountingRelease>;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

static bool released_are(std::vector<int> want) {
  const bool same = g_released == want;
  g_released.clear();
  return same;
}

static int takes_handle(int h) { return h; }

int main() {
  const long live0 = axw::live_owned.load();

  {  // an empty owner releases nothing
    Own e;
    CHECK(e.get() == 0 && !e);
    CHECK(axw::live_owned == live0);
  }
  CHECK(released_are({}));

  {  // acquire, destroy: one release, with the handle it was given
    Own a(41);
    CHECK(a.get() == 41 && takes_handle(a) == 41);  // converts implicitly
    CHECK(axw::live_owned == live0 + 1);
    CHECK(released_are({}));
  }
  CHECK(released_are({41}));
  CHECK(axw::live_owned == live0);

  {  // move construction: the handle moves, the source's destructor releases nothing
    Own a(1);
    {
      Own b(std::move(a));
      CHECK(a.get() == 0 && b.get() == 1);
      CHECK(axw::live_owned == live0 + 1);
    }
    CHECK(released_are({1}));
  }
  CHECK(released_are({}));

  {  // move assignment: the target's old handle is released exactly once, then it holds the source's
    Own a(2), b(3);
    b = std::move(a);
    CHECK(released_are({3}));
    CHECK(a.get() == 0 && b.get() == 2);
    CHECK(axw::live_owned == live0 + 1);
  }
  CHECK(released_are({2}));

  {  // self-move-assignment keeps the handle
    Own a(4);
    Own& alias = a;
    a = std::move(alias);
    CHECK(a.get() == 4);
    CHECK(released_are({}));
    CHECK(axw::live_owned == live0 + 1);
  }
  CHECK(released_are({4}));

  {  // reset(h) releases the old handle; release() releases nothing
    Own a(5);
    a.reset(6);
    CHECK(released_are({5}));
    CHECK(a.get() == 6 && axw::live_owned == live0 + 1);
    CHECK(a.release() == 6);
    CHECK(a.get() == 0 && axw::live_owned == live0);
    a.reset();  // empty: nothing
    CHECK(released_are({}));
  }
  CHECK(released_are({}));

  {  // containers: clear() and erase() release each element once
    std::vector<Own> v;
    for (int i = 10; i < 14; ++i) v.emplace_back(i);  // (grows: elements are moved, not released)
    CHECK(released_are({}));
    CHECK(axw::live_owned == live0 + 4);
    v.clear();
    CHECK(released_are({10, 11, 12, 13}));
    std::map<long, Own> m;
    m[7] = Own(20);
    m[8] = Own(21);
    CHECK(released_are({}));
    m.erase(7);
    CHECK(released_are({20}));
    m[8] = Own(22);  // replacing an entry releases what it held
    CHECK(released_are({21}));
    m.clear();
    CHECK(released_are({22}));
    CHECK(axw::live_owned == live0);
  }

  {  // five acquisitions, a throw after the third: those three are released (last first) and nothing else
    struct Five {
      Own a, b, c, d, e;
      Five() {
        a = Own(31);
        b = Own(32);
        c = Own(33);
        throw std::runtime_error("after the third");
        d = Own(34);
        e = Own(35);
      }
    };
    bool thrown = false;
    try {
      Five f;
    } catch (const std::runtime_error&) {
      thrown = true;
    }
    CHECK(thrown);
    CHECK(released_are({33, 32, 31}));
  }

  CHECK(axw::live_owned == live0);
  printf("owned ok\n");
  return 0;
}

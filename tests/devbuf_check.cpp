// DevBuf<T> (csrc/svr_devbuf.h) on counting stand-ins for hipMalloc / hipFree over malloc / free: what reserve, reset, the moves and the
// destructor promise, the failure path included, without a device.  tests/test_abi.py builds it with -fsanitize=address,undefined and
// runs it; it prints "ok" and returns 0, or says which line failed.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
namespace {
int n_alloc = 0, n_free = 0;
bool fail_next = false;                 // the next allocation fails (once)
std::vector<char> events;               // 'a' / 'f' in call order
size_t last_bytes = 0;
}  // namespace
hipError_t hipMalloc(void **p, size_t bytes) {
  if (fail_next) { fail_next = false; *p = nullptr; return hipErrorOutOfMemory; }
  *p = malloc(bytes ? bytes : 1);
  ++n_alloc; last_bytes = bytes; events.push_back('a');
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  if (p) { free(p); ++n_free; events.push_back('f'); }
  return hipSuccess;
}

#include "../fetalreconstruction_amd/csrc/svr_devbuf.h"

#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

struct Rec { double a; int b; };        // 16 bytes

static int checks() {
  {
    DevBuf<float> b;
    CHECK(b.get() == nullptr && b.capacity() == 0 && !b);
    CHECK(b.reserve(0) == hipSuccess && n_alloc == 0);                      // nothing asked for, nothing allocated
    CHECK(b.reserve(10) == hipSuccess && n_alloc == 1 && last_bytes == 10 * sizeof(float) && b.capacity() == 10 && b.get());
    float *p = b;                                                           // the implicit conversion
    CHECK(p == b.get());
    p[9] = 1.0f;                                                            // (the sanitizer checks the size)
    // at or below the capacity: no allocation, the same block
    CHECK(b.reserve(10) == hipSuccess && b.reserve(3) == hipSuccess && n_alloc == 1 && n_free == 0 && b.get() == p && b.capacity() == 10);
    // growth: the old block is freed BEFORE the new one is asked for, and the request is exactly n * sizeof(T)
    events.clear();
    CHECK(b.reserve(11) == hipSuccess && n_alloc == 2 && n_free == 1 && last_bytes == 11 * sizeof(float) && b.capacity() == 11);
    CHECK(events.size() == 2 && events[0] == 'f' && events[1] == 'a');
    CHECK(b.reserve(1000003) == hipSuccess && last_bytes == 1000003 * sizeof(float) && b.capacity() == 1000003);   // no rounding, no doubling
    // a failed growth: empty, capacity 0, the old block gone; the next reserve works
    fail_next = true;
    const int before_alloc = n_alloc, before_free = n_free;
    CHECK(b.reserve(2000000) == hipErrorOutOfMemory && b.get() == nullptr && b.capacity() == 0 && n_alloc == before_alloc && n_free == before_free + 1);
    CHECK(b.reserve(5) == hipSuccess && b.capacity() == 5 && b.get() && last_bytes == 5 * sizeof(float));
    // reset, twice
    b.reset();
    CHECK(b.get() == nullptr && b.capacity() == 0 && n_alloc == n_free);
    b.reset();
    CHECK(n_alloc == n_free);
    fail_next = true;                                                       // a failure on an empty buffer frees nothing
    CHECK(b.reserve(1) != hipSuccess && !b && n_alloc == n_free);
  }
  {
    DevBuf<Rec> r;
    CHECK(r.reserve(7) == hipSuccess && last_bytes == 7 * sizeof(Rec));
    DevBuf<unsigned char> bytes;
    CHECK(bytes.reserve(33) == hipSuccess && last_bytes == 33);
    DevBuf<void> v;                                                         // a byte arena
    CHECK(v.reserve(17) == hipSuccess && last_bytes == 17 && v.capacity() == 17);
    void *q = v;
    CHECK(q == v.get());
  }                                                                         // the destructors free
  CHECK(n_alloc == n_free);
  {
    // move construction: the source is empty, nothing is allocated or freed
    DevBuf<int> a;
    CHECK(a.reserve(4) == hipSuccess);
    int *pa = a;
    const int al = n_alloc, fr = n_free;
    DevBuf<int> b(std::move(a));
    CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == pa && b.capacity() == 4 && n_alloc == al && n_free == fr);
    // move assignment: the destination's old block is freed, the source is empty
    DevBuf<int> c;
    CHECK(c.reserve(9) == hipSuccess);
    const int fr2 = n_free;
    c = std::move(b);
    CHECK(n_free == fr2 + 1 && c.get() == pa && c.capacity() == 4 && b.get() == nullptr && b.capacity() == 0);
    DevBuf<int> &self = c;
    c = std::move(self);                                                    // onto itself: untouched
    CHECK(c.get() == pa && c.capacity() == 4);
    std::swap(a, c);                                                        // (the engine swaps two of its buffers)
    CHECK(a.get() == pa && a.capacity() == 4 && !c);
    CHECK(a.reserve(2) == hipSuccess && a.get() == pa);                     // the emptied and the refilled both still work
    CHECK(c.reserve(2) == hipSuccess && c.get());
  }
  CHECK(n_alloc == n_free && n_alloc > 0);
  static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "DevBuf is move-only");
  return 0;
}

int main() {
  const int r = checks();
  if (r) return r;
  printf("ok: %d allocations, %d frees\n", n_alloc, n_free);
  return n_alloc == n_free ? 0 : 1;
}

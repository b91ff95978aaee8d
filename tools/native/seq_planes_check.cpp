// The bookkeeping of mfx_seq_planes_once (csrc/mfx_internal.h) -- the packed planes a resident sequence gets once, and the fall back to one
// byte per base when they cannot be had -- without a device: the allocator, the release and the fill are this program's, every way they
// can fail is taken, and every allocation is a host block, so AddressSanitizer sees a leak, a double release or a use after one.
//   g++ -fsanitize=address,undefined -std=c++17 -I merfin_amd/csrc -I include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/native/seq_planes_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "mfx_internal.h"

static std::set<void *> live;
static int bad = 0;
#define CHECK(x) do { if (!(x)) { printf("MISMATCH %s:%d: %s\n", __FILE__, __LINE__, #x); ++bad; } } while (0)

struct Plan { int fail_alloc; bool fail_fill; };     // fail_alloc: the n-th allocation (1, 2) fails; 0: none

// one run: returns what mfx_seq_planes_once said; *allocs / *fills: the calls it made
static bool run(mfx_seq *s, uint64_t pw, Plan p, int *allocs, int *fills) {
  int na = 0, nf = 0;
  const bool r = mfx_seq_planes_once(
      s, pw,
      [&](void **q, size_t bytes) {
        if (++na == p.fail_alloc) { *q = nullptr; return false; }
        *q = malloc(bytes);
        memset(*q, 0xAB, bytes);
        live.insert(*q);
        return true;
      },
      [&](void *q) { CHECK(live.erase(q) == 1); free(q); },
      [&](mfx_seq *t) {
        ++nf;
        CHECK(t->d_codes && t->d_valid);                       // the fill sees both planes
        if (p.fail_fill) return false;
        memset(t->d_codes, 0, pw * sizeof(uint64_t));          // (the whole of each plane is the sequence's: ASan checks the sizes)
        memset(t->d_valid, 0, pw * sizeof(uint32_t));
        return true;
      });
  *allocs = na;
  *fills = nf;
  return r;
}

int main() {
  const uint64_t pw = 131 + 7;
  int na, nf, cases = 0;
  uint8_t bases_tag = 0;
  // every way to fail, then success: the sequence stays ASCII, owns nothing, and a later call may still succeed
  for (const Plan p : {Plan{1, false}, Plan{2, false}, Plan{0, true}, Plan{0, false}}) {
    mfx_seq s;
    s.d_bases = &bases_tag;
    const bool r = run(&s, pw, p, &na, &nf);
    const bool want = p.fail_alloc == 0 && !p.fail_fill;
    CHECK(r == want && s.planes_ok == want);
    CHECK(!s.bases_stale && s.d_bases == &bases_tag);          // d_bases stays, and stays current
    CHECK((s.d_codes != nullptr) == want && (s.d_valid != nullptr) == want);
    CHECK(live.size() == (want ? 2u : 0u));
    CHECK(na == (p.fail_alloc == 1 ? 1 : 2) && nf == (p.fail_alloc ? 0 : 1));
    if (!want) {                                               // ... and the same object again, with room this time
      CHECK(run(&s, pw, Plan{0, false}, &na, &nf) && s.planes_ok && na == 2 && nf == 1 && live.size() == 2);
    }
    CHECK(run(&s, pw, Plan{1, true}, &na, &nf) && na == 0 && nf == 0);      // planes there: nothing is made again
    for (void *q : {(void *)s.d_codes, (void *)s.d_valid}) { CHECK(live.erase(q) == 1); free(q); }
    printf("case alloc-fails-at %d, fill %s: planes_ok %d\n", p.fail_alloc, p.fail_fill ? "fails" : "works", (int)want);
    ++cases;
  }
  {
    // planes a streamed run left behind (allocated, not current): reused, not allocated again; released when the fill fails
    for (const bool ff : {false, true}) {
      mfx_seq s;
      s.d_bases = &bases_tag;
      s.d_codes = (uint64_t *)malloc(pw * 8); live.insert(s.d_codes);
      s.d_valid = (uint32_t *)malloc(pw * 4); live.insert(s.d_valid);
      const bool r = run(&s, pw, Plan{1, ff}, &na, &nf);
      CHECK(r == !ff && s.planes_ok == !ff && na == 0 && nf == 1);
      CHECK(live.size() == (ff ? 0u : 2u) && (s.d_codes != nullptr) == !ff && (s.d_valid != nullptr) == !ff);
      if (!ff) for (void *q : {(void *)s.d_codes, (void *)s.d_valid}) { CHECK(live.erase(q) == 1); free(q); }
      printf("case planes left behind, fill %s\n", ff ? "fails" : "works");
      ++cases;
    }
  }
  {
    // a packed upload (the planes ARE the sequence, d_bases stale or absent): untouched
    mfx_seq s;
    s.bases_stale = true;
    CHECK(run(&s, pw, Plan{1, true}, &na, &nf) && na == 0 && nf == 0 && s.bases_stale && !s.d_codes);
    printf("case packed upload\n");
    ++cases;
  }
  CHECK(live.empty());
  printf("%s (%d mismatches, %d cases)\n", bad ? "FAILED" : "OK", bad, cases);
  return bad ? 1 : 0;
}

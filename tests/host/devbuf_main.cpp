// Host-only check of DevBuf (csrc/dto_problem.hpp): the HIP allocation calls are replaced by malloc / free / memset stubs with a
// live-allocation counter and a switch that fails the next allocation above a given size.  Built without the HIP runtime and run
// under the address and undefined-behaviour sanitizers by tests/test_devbuf_host.py; exit status 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "../../directtrajectoryoptimization.jl_amd/csrc/dto_problem.hpp"

static long g_live = 0;                    // allocations made and not yet freed
static size_t g_fail_above = (size_t)-1;   // the next hipMalloc of more bytes than this fails (once)

hipError_t hipMalloc(void** p, size_t bytes) {
  if (bytes > g_fail_above) { g_fail_above = (size_t)-1; *p = (void*)0x10; return hipErrorOutOfMemory; }   // (a pointer nobody may keep)
  *p = malloc(bytes);
  memset(*p, 0xA5, bytes);   // device memory is not zero-filled
  ++g_live;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (p) { free(p); --g_live; }
  return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t bytes) {
  memset(p, v, bytes);
  return hipSuccess;
}

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

using dto::DevBuf;

int main() {
  {
    DevBuf<double> a;
    CHECK((double*)a == nullptr && a.size() == 0 && g_live == 0);
    a.reset();   // an empty buffer frees nothing
    CHECK(g_live == 0);

    // alloc does not initialise, alloc_zeroed zeroes every element
    CHECK(a.alloc(100) == hipSuccess && a.size() == 100 && g_live == 1);
    unsigned char raw;
    memcpy(&raw, (double*)a, 1);
    CHECK(raw == 0xA5);
    CHECK(a.alloc_zeroed(100) == hipSuccess && a.size() == 100 && g_live == 1);   // the first block was released
    for (size_t i = 0; i < a.size(); ++i) CHECK(a[i] == 0.0);

    // grow: at or below the capacity the pointer stays, above it the block is replaced (contents not kept)
    double* p0 = a;
    a[7] = 3.0;
    CHECK(a.grow(0) == hipSuccess && a.grow(50) == hipSuccess && a.grow(100) == hipSuccess && (double*)a == p0 && a.size() == 100 && a[7] == 3.0);
    CHECK(a.grow(101) == hipSuccess && a.size() == 101 && g_live == 1);
    CHECK(a[7] != 3.0);   // a new, unfilled block
    DevBuf<int> e;
    CHECK(e.grow(0) == hipSuccess && (int*)e == nullptr && g_live == 1);   // nothing asked for, nothing allocated

    // a failed alloc / alloc_zeroed / grow: the old block is gone, the buffer is empty, the error comes back
    g_fail_above = 1000;
    CHECK(a.alloc(1000) == hipErrorOutOfMemory && (double*)a == nullptr && a.size() == 0 && g_live == 0);
    CHECK(a.alloc(10) == hipSuccess && g_live == 1);
    g_fail_above = 1000;
    CHECK(a.grow(1000) == hipErrorOutOfMemory && (double*)a == nullptr && a.size() == 0 && g_live == 0);
    g_fail_above = 1000;
    CHECK(a.alloc_zeroed(1000) == hipErrorOutOfMemory && (double*)a == nullptr && a.size() == 0 && g_live == 0);
    CHECK(a.grow(10) == hipSuccess && a.size() == 10 && g_live == 1);   // the switch fails one allocation only: a retry succeeds

    // alloc(0) gives one element, so that "is it allocated" can be read from the pointer
    DevBuf<int> z;
    CHECK(z.alloc(0) == hipSuccess && (int*)z != nullptr && z.size() == 1 && g_live == 2);
    CHECK(z.alloc_zeroed(0) == hipSuccess && z[0] == 0 && g_live == 2);

    // move construction and move assignment leave the source empty; assignment frees what the target held
    double* pa = a;
    DevBuf<double> b(std::move(a));
    CHECK((double*)b == pa && b.size() == 10 && (double*)a == nullptr && a.size() == 0 && g_live == 2);
    DevBuf<double> c;
    CHECK(c.alloc(5) == hipSuccess && g_live == 3);
    c = std::move(b);
    CHECK((double*)c == pa && c.size() == 10 && (double*)b == nullptr && b.size() == 0 && g_live == 2);
    DevBuf<double>& self = c;
    c = std::move(self);
    CHECK((double*)c == pa && c.size() == 10 && g_live == 2);

    // std::swap (dto_solver_iterate swaps z / z_alt), with an empty partner too
    DevBuf<double> d;
    CHECK(d.alloc(3) == hipSuccess && g_live == 3);
    double* pd = d;
    std::swap(c, d);
    CHECK((double*)c == pd && c.size() == 3 && (double*)d == pa && d.size() == 10 && g_live == 3);
    DevBuf<double> none;
    std::swap(c, none);
    CHECK((double*)c == nullptr && c.size() == 0 && (double*)none == pd && none.size() == 3 && g_live == 3);

    // the conversion: pointer arithmetic, truth value, a const-qualified destination
    const double* cd = d;
    CHECK(cd == pa && d + 2 == pa + 2 && d && !c);
    d.reset();
    CHECK((double*)d == nullptr && d.size() == 0 && g_live == 2);
  }
  CHECK(g_live == 0);   // every destructor freed its block, none twice (the sanitizer watches the second half)
  if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
  printf("devbuf ok\n");
  return 0;
}

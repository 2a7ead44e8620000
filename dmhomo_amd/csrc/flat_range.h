// The flat range of a [B][n] fp32 tensor as a scalar head, 16-byte vectors and a scalar tail, for the in-place row kernels
// that shift logits (flowg.hip, pag.hip): grid-stride launches of FT threads, at most F_MAX_WG workgroups.
#pragma once
#include "common.h"

constexpr int FT = 256;          // threads of a workgroup
constexpr int F_MAX_WG = 2048;   // workgroups of a launch: 8 per CU, the rest of the elements by the grid stride

// the row of flat element i: 32-bit division where the whole tensor has fewer than 2^32 elements (uniform over the launch)
__device__ __forceinline__ int64_t row_of(int64_t i, int64_t n, bool small) {
  return small ? (int64_t)((uint32_t)i / (uint32_t)n) : i / n;
}

// The flat range [0, total) as a scalar head [0, head), nv 16-byte vectors from head on, and a scalar tail: head brings the
// pointers (which share their 16-byte phase, or nv == 0 and head == total) to a 16-byte boundary.
struct FlatSplit {
  int64_t head, nv, t0;
};

static FlatSplit flat_split(const void* p, int64_t total, bool same_phase) {
  FlatSplit s;
  if (!same_phase) {
    s.head = total, s.nv = 0, s.t0 = total;
    return s;
  }
  const int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
  s.head = head < total ? head : total;
  s.nv = (total - s.head) >> 2;
  s.t0 = s.head + s.nv * 4;
  return s;
}

static unsigned flat_grid(const FlatSplit& s, int64_t total) {
  const int64_t scalar = s.head + (total - s.t0);
  const int64_t g = cdiv64(s.nv > scalar ? s.nv : scalar, FT);
  return (unsigned)(g < F_MAX_WG ? (g > 0 ? g : 1) : F_MAX_WG);
}

// argument checks of the entries
static bool rows_ok(const char* who, int B, int64_t n) {
  if (B < 1 || n < 1 || n >= ((int64_t)1 << 31)) {
    dmh_set_error("%s: B=%d rows of n=%lld elements (B >= 1, 1 <= n < 2^31)", who, B, (long long)n);
    return false;
  }
  return true;
}

static bool overlaps(const void* a, const void* b, uintptr_t bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && pa < pb + bytes && pb < pa + bytes;
}

static bool same_phase(const void* a, const void* b) { return !b || (((uintptr_t)a ^ (uintptr_t)b) & 15u) == 0; }

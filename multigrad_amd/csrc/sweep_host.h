// Host scaffolding of the optimizer vector kernels (gram.hip, box_dual.hip, lbfgs.hip,
// hmc.hip): the 16-byte alignment test every translation unit uses, the resident-workgroup
// cap of a grid-stride launch, the grid it gives, and the row-tile dispatch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

namespace mg {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Workgroups of `threads` threads that the current device holds resident at once, for the
// kernel of `kernels` with the least occupancy, at most max_blocks: CUs x occupancy.  A
// grid-stride launch capped there starts no workgroup after the first ones have finished,
// and kernels that share a cap launch the same grid and so sum in the same order.  The
// occupancy query costs host time, so the answer is kept per device in the caller's GridCap.
constexpr int kCapDevices = 64;
struct GridCap {
  int v[kCapDevices] = {};
};

template <typename... K>
int resident_cap(GridCap& cap, int max_blocks, int threads, K... kernels) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const bool keep = dev >= 0 && dev < kCapDevices;
  if (keep && cap.v[dev] != 0) return cap.v[dev];
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  int per = 1 << 30;
  auto one = [&](auto k) {
    int v = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k, threads, 0);
    per = std::min(per, std::max(1, v));
  };
  (one(kernels), ...);
  const int c = std::max(1, std::min(max_blocks, std::max(1, cus) * per));
  if (keep) cap.v[dev] = c;
  return c;
}

// Work items of a column sweep over n columns: float4 groups plus the n % 4 single columns,
// or n single columns.
inline int64_t sweep_chunks(int64_t n, bool vec) { return vec ? (n >> 2) + (n & 3) : n; }

// Grid of a grid-stride launch: one thread per chunk, at least 1 and at most cap workgroups.
inline int chunk_grid(int64_t chunks, int threads, int64_t cap) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((chunks + threads - 1) / threads, cap));
}

// f(std::integral_constant<int, T>) for the least row tile T of 1, 2, 4, 8, 10(, 16) that
// holds K <= MAXT rows.
template <int MAXT, typename F>
void dispatch_row_tile(int K, F&& f) {
  static_assert(MAXT == 10 || MAXT == 16, "the ladder ends at 10 or 16");
  if (K <= 1) f(std::integral_constant<int, 1>{});
  else if (K <= 2) f(std::integral_constant<int, 2>{});
  else if (K <= 4) f(std::integral_constant<int, 4>{});
  else if (K <= 8) f(std::integral_constant<int, 8>{});
  else if (MAXT == 10 || K <= 10) f(std::integral_constant<int, 10>{});
  else if constexpr (MAXT == 16) f(std::integral_constant<int, 16>{});
}

}  // namespace mg

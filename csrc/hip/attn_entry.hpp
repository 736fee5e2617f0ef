// Host side of the attention path: what the extern "C" entry points of
// decode_kernels.hip and prefill_kernels.hip share.
#ifndef GPBS_HIP_ATTN_ENTRY_HPP
#define GPBS_HIP_ATTN_ENTRY_HPP

#include <algorithm>
#include <climits>
#include <initializer_list>
#include <type_traits>

#include "attn_cache.hpp"

namespace gpbs_hip {

// log2(page) for the page sizes the paged kernels take, -1 otherwise
inline int page_shift(int page) { return page == 64 ? 6 : page == 128 ? 7 : page == 256 ? 8 : -1; }

// what a paged entry point refuses of its cache geometry
inline bool bad_pages(int NP, int P, int psh) {
  return NP < 1 || P < 1 || psh < 0 || ((long long)NP << psh) > INT_MAX;
}

inline bool any_null(std::initializer_list<const void*> ps) {
  return std::any_of(ps.begin(), ps.end(), [](const void* p) { return !p; });
}

// the return code of an entry point after its launches
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -5; }

// launch(g) with g = std::integral_constant<int, G> for the group sizes the
// attention kernels are built for; false, and no call, for any other G
template <class Launch>
bool for_group(int G, Launch launch) {
  switch (G) {
    case 1: launch(std::integral_constant<int, 1>()); return true;
    case 2: launch(std::integral_constant<int, 2>()); return true;
    case 4: launch(std::integral_constant<int, 4>()); return true;
    case 8: launch(std::integral_constant<int, 8>()); return true;
    default: return false;
  }
}

// a write kernel over n8 16-byte pieces of qkv rows: one thread per piece,
// grid-stride from at most max_grid workgroups of kWriteThreads (the stride the
// write templates assume)
template <class Kernel, class... Args>
int launch_write(Kernel kernel, size_t n8, int max_grid, hipStream_t s, Args... args) {
  const int grid = (int)std::min<size_t>((n8 + kWriteThreads - 1) / kWriteThreads, max_grid);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kWriteThreads), 0, s, args...);
  return launched();
}

}  // namespace gpbs_hip

#endif  // GPBS_HIP_ATTN_ENTRY_HPP

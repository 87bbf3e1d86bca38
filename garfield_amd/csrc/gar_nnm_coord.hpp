// Nearest-neighbour mixing in front of a coordinate-wise rule: pieces shared by the translation
// units of k_nnm_coord (gar_nnm_coord.hip: the sets launch, the LDS form and the dispatcher;
// gar_nnm_coord_mfma.hip: the MFMA form).
#pragma once
#include "gar_bulyan_tail.hpp"

namespace garfield {
namespace gpu {
namespace coord {

typedef unsigned long long u64;

// The rule over the n mixed values of one coordinate, held by one lane (v[k], k >= nn: anything).
// coord_reduce's conventions: trimmed mean sorts with NaN as +inf, drops ff at each end and averages
// the nn - 2 ff others; median is the upper median of the finite values, 0 if there is none. nn and
// ff are wave-uniform.
template <int NP, int MODE>
__device__ __forceinline__ float nnm_rule(float (&v)[NP], int nn, int ff) {
  static_assert(MODE == kTrimmedMean || MODE == kMedian, "nnm_rule: trimmed mean or median");
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    if constexpr (MODE == kMedian) {
      const bool ok = (k < nn) && isfinite(v[k]);
      cnt += ok;
      v[k] = ok ? v[k] : kInf;
    } else {
      v[k] = (k < nn) ? sanitize_inf(v[k]) : kInf;
    }
  }
  oem_sort_f32<NP>(v);
  if constexpr (MODE == kMedian) {
    const float med = pick_sel(v, cnt >> 1);
    return cnt ? med : 0.f;
  } else {
    const int hi = nn - ff;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) s += (i >= ff && i < hi) ? v[i] : 0.f;
    return s / static_cast<float>(nn - 2 * ff);
  }
}

// bf16 / fp16 rows, n <= 64: the n set sums on MFMA (gar_nnm_coord_mfma.hip)
void launch_nnm_coord_mfma(const RowTable& rows, int n, int64_t d, int dt, int mode, int f, const u64* masks,
                           void* out, int out_dt, hipStream_t s);

}  // namespace coord
}  // namespace gpu
}  // namespace garfield

// Dispatcher of the coordinate-wise rules.
#include "gar_coord.hpp"

namespace garfield {
namespace gpu {

namespace coord {
template <> void coord_mode<kMedian>(int, const Plan&, const RowTable&, int, int64_t, int, int, const float*, int,
                               uint64_t, uint64_t, void*, int, hipStream_t);
template <> void coord_mode<kTrimmedMean>(int, const Plan&, const RowTable&, int, int64_t, int, int, const float*, int,
                               uint64_t, uint64_t, void*, int, hipStream_t);
template <> void coord_mode<kAveragedMedian>(int, const Plan&, const RowTable&, int, int64_t, int, int, const float*, int,
                               uint64_t, uint64_t, void*, int, hipStream_t);
template <> void coord_mode<kAverageNan>(int, const Plan&, const RowTable&, int, int64_t, int, int, const float*, int,
                               uint64_t, uint64_t, void*, int, hipStream_t);
template <> void coord_mode<kCondense>(int, const Plan&, const RowTable&, int, int64_t, int, int, const float*, int,
                               uint64_t, uint64_t, void*, int, hipStream_t);
template <> void coord_mode<kBulyanTail>(int, const Plan&, const RowTable&, int, int64_t, int, int, const float*, int,
                               uint64_t, uint64_t, void*, int, hipStream_t);
}  // namespace coord

int coordwise_max_rows() { return kMaxRows; }

CoordPlanInfo coordwise_plan(int n, int64_t d, int dt, int mode, int f, int beta, int t, bool has_W) {
  const coord::Plan pl = coord::plan(dt, mode, n, d, f, beta, t, has_W);
  return {coord::family_name(pl.family), pl.np, pl.grid, pl.coords_per_pass, pl.sub};
}

void coordwise(const RowTable& rows, int n, int64_t d, int dt, int mode, int f, int beta, const float* W, int t,
               uint64_t seed, uint64_t threshold, void* out, int out_dt, hipStream_t stream) {
  const coord::Plan pl = coord::plan(dt, mode, n, d, f, beta, t, W != nullptr);
  switch (mode) {
    case kMedian: coord::coord_mode<kMedian>(dt, pl, rows, n, d, f, beta, W, t, seed, threshold, out, out_dt, stream); break;
    case kTrimmedMean: coord::coord_mode<kTrimmedMean>(dt, pl, rows, n, d, f, beta, W, t, seed, threshold, out, out_dt, stream); break;
    case kAveragedMedian: coord::coord_mode<kAveragedMedian>(dt, pl, rows, n, d, f, beta, W, t, seed, threshold, out, out_dt, stream); break;
    case kAverageNan: coord::coord_mode<kAverageNan>(dt, pl, rows, n, d, f, beta, W, t, seed, threshold, out, out_dt, stream); break;
    case kCondense: coord::coord_mode<kCondense>(dt, pl, rows, n, d, f, beta, W, t, seed, threshold, out, out_dt, stream); break;
    default: coord::coord_mode<kBulyanTail>(dt, pl, rows, n, d, f, beta, W, t, seed, threshold, out, out_dt, stream); break;
  }
}

}  // namespace gpu
}  // namespace garfield

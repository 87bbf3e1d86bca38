// Which kernel a coordinate-wise rule runs on: ONE pure host function, coord::plan, holds every
// run-time condition of the dispatch (dtype, padded row count, n, t, t - beta, window_mean's
// spilled positions, the process-wide knobs) and the launch grid. launch_coord and the tail
// launchers obey its answer; the binding _C.coord_plan shows it to the tests. No device code here.
#pragma once
#include <cstdint>
#include <cstdlib>
#include "gar_common.hpp"

namespace garfield {
namespace gpu {
namespace coord {

// knobs (read once per process): GARFIELD_COORD16=0 disables the packed 16-bit-key kernels and
// the tail kernels (A/B runs); GARFIELD_COORD16_GRID caps the packed kernels' grid
inline bool coord16_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("GARFIELD_COORD16");
    return !(e && e[0] == '0');
  }();
  return on;
}
inline bool coord_mfma_tail_enabled() {  // GARFIELD_MFMA_TAIL=0: Bulyan tail without MFMA (A/B runs)
  static const bool on = [] {
    const char* e = std::getenv("GARFIELD_MFMA_TAIL");
    return !(e && e[0] == '0');
  }();
  return on;
}
// Grid cap of the packed 16-bit coordinate kernels (grid-stride loop). Measured at d = 23.5M
// bf16 (profiles/r2/coord16_grid_sweep.log): small sets (NP <= 16, 8 coordinates per lane) are
// fastest with one pass per lane (cap 16384: median n=8 0.080 vs 0.084 ms at 4096); large sets
// with 4096 (n=64 0.611 vs 0.634 ms at 16384). GARFIELD_COORD16_GRID overrides both.
inline int64_t coord16_grid_cap(int np) {
  static const int64_t env = [] {
    const char* e = std::getenv("GARFIELD_COORD16_GRID");
    const long v = e ? std::atol(e) : 0;
    return static_cast<int64_t>(v > 0 ? v : 0);
  }();
  if (env > 0) return env;
  return np <= 16 ? 16384 : 4096;
}
// grid cap of the tail kernels (grid-stride over coordinate groups); GARFIELD_TAIL_GRID overrides
inline int64_t tail_grid_cap(int64_t dflt) {
  static const int64_t env = [] {
    const char* e = std::getenv("GARFIELD_TAIL_GRID");
    const long v = e ? std::atol(e) : 0;
    return static_cast<int64_t>(v > 0 ? v : 0);
  }();
  return env > 0 ? env : dflt;
}

inline int np_for(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : (k <= 32 ? 32 : (k <= 64 ? 64 : 128))); }

constexpr int kCoordTile = 256;       // coordinates per LDS tile of k_coordwise_lds
constexpr int kTailTile = 256;        // coordinates per LDS tile of k_bulyan_tail
constexpr int kTailMaxExcluded = 16;  // the window kernels hold e = t - beta <= 16 excluded values
// window_mean (gar_bulyan_tail.hpp) reads the sorted positions t / 2 and beta .. t - 1 from an LDS
// spill that starts at P0 = wm_p0(NP): both must be >= P0
constexpr int wm_p0(int np) { return (np / 4) & ~3; }

constexpr int coord_vec(int np) { return np <= 8 ? 8 : (np <= 16 ? 4 : (np <= 32 ? 2 : 1)); }    // k_coordwise
constexpr int coord16_words(int np) { return np <= 16 ? 4 : (np == 32 ? 2 : 1); }                 // k_coord16
constexpr bool coord16_mode(int mode) { return mode == kMedian || mode == kTrimmedMean || mode == kCondense; }

enum Family : int {
  kFamCoord16 = 0,        // k_coord16                 (gar_coord16.hpp)
  kFamCoordwise,          // k_coordwise               (gar_coord.hpp)
  kFamCoordwiseLds,       // k_coordwise_lds           (gar_coord.hpp)
  kFamTailWindow,         // k_bulyan_tail<.., false>  (gar_bulyan_tail.hpp)
  kFamTailWindowDirect,   // k_bulyan_tail<.., true>   (gar_bulyan_tail.hpp)
  kFamTailMfma,           // k_bulyan_tail_mfma        (gar_bulyan_tail.hpp)
  kFamTailF32,            // k_bulyan_tail_f32         (gar_tail_f32.hip)
};

inline const char* family_name(int fam) {
  switch (fam) {
    case kFamCoord16: return "coord16";
    case kFamCoordwise: return "coordwise";
    case kFamCoordwiseLds: return "coordwise_lds";
    case kFamTailWindow: return "tail_window";
    case kFamTailWindowDirect: return "tail_window_direct";
    case kFamTailMfma: return "tail_mfma";
    default: return "tail_f32";
  }
}

struct Plan {
  int family;               // Family
  int np;                   // padded row (set) count the kernel is instantiated for
  int64_t grid;             // workgroups (256 threads each)
  int64_t coords_per_pass;  // coordinates ONE workgroup covers per pass of its grid-stride loop:
                            // grid * coords_per_pass < d  <=>  the loop wraps
  int sub;                  // the family's second template choice: VEC (coordwise), words per row P
                            // (coord16), MFMA k-steps KS (tail_mfma), padded rows NR (tail_f32); else 0
};

inline int64_t clamp_grid(int64_t g, int64_t cap) {
  if (g > cap) g = cap;
  return g < 1 ? 1 : g;
}

// mode is what coordwise() receives (after the binding's averaged-median reroute); has_W: a
// selection matrix W[t, n] is given (Bulyan's tail)
inline Plan plan(int dt, int mode, int n, int64_t d, int f, int beta, int t, bool has_W) {
  (void)f;
  const bool bulyan = mode == kBulyanTail;
  const int np = np_for(bulyan ? t : n);
  const int esz = dt == kF32 ? 4 : 2;
  // packed 16-bit keys: median / trimmed mean / condense on bf16 / fp16
  if (dt != kF32 && coord16_mode(mode) && coord16_enabled()) {
    const int P = coord16_words(np);
    return {kFamCoord16, np, clamp_grid((d / (2 * P) + 255) / 256, coord16_grid_cap(np)), 256 * 2 * P, P};
  }
  // Bulyan's tail in registers: n, t <= 64, e <= 16 and window_mean's spilled positions
  const bool wm_ok = bulyan && has_W && n <= 64 && t <= 64 && t >= 1 && beta >= 1 && t - beta <= kTailMaxExcluded &&
                     t / 2 >= wm_p0(np) && beta >= wm_p0(np) && coord16_enabled();
  if (wm_ok && dt != kF32 && coord_mfma_tail_enabled())
    return {kFamTailMfma, np, clamp_grid((d / 64 + 3) / 4, tail_grid_cap(4096)), 256, (n + 15) / 16};
  if (wm_ok && dt == kF32 && d >= 1)
    return {kFamTailF32, np, clamp_grid(((d + 63) / 64 + 3) / 4, tail_grid_cap(2048)), 256,
            n <= 16 ? 16 : (n <= 32 ? 32 : 64)};
  // the window kernel on an LDS tile: any t <= 64 sets (or the n rows themselves) with e <= 16
  if ((bulyan || mode == kAveragedMedian) && np <= 64 && n <= 64 && (bulyan ? t : n) - beta <= kTailMaxExcluded &&
      coord16_enabled()) {
    int64_t g = d / kTailTile + 1;
    const int64_t cap = tail_grid_cap(4096);
    if (g > cap) g = cap;
    return {bulyan && has_W ? kFamTailWindow : kFamTailWindowDirect, np, g, kTailTile, 0};
  }
  // LDS-staged generic kernel: NP >= 32, tile <= 64 KB, and (Bulyan's tail) all n rows fit the NP-row tile
  if (np >= 32 && np * kCoordTile * esz <= 65536 && (!bulyan || n <= np))
    return {kFamCoordwiseLds, np, clamp_grid(d / kCoordTile, 2048), kCoordTile, 0};
  const int vec = coord_vec(np);
  return {kFamCoordwise, np, clamp_grid((d / vec + 255) / 256, 4096), 256 * vec, vec};
}

}  // namespace coord
}  // namespace gpu
}  // namespace garfield

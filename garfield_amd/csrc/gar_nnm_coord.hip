// Nearest-neighbour mixing (NNM) in front of a coordinate-wise rule (trimmed mean, median).
//
// A coordinate-wise rule has no weight vector to fold the mixing into: per coordinate x it needs the n
// mixed values y_i[x] = (1/c) Σ_{j∈S_i} x_j[x] (c = n - f) and an order statistic over them. The mixed
// rows are never stored: one pass reads the n rows and writes d values (docs/GAR_SEMANTICS.md
// "Nearest-neighbour mixing before a coordinate-wise rule").
//
//  k_nnm_sets   masks[n][2] from the Gram: the rank count + ballot of k_nnm_mix without its pseudo-Gram
//               (dev::nnm_build_sets, shared by both kernels: the same sets, bit for bit).
//  k_nnm_coord  the n set means and the rule, per coordinate. Two forms, picked by (dtype, n) only:
//               bf16 / fp16 rows with n <= 64 on MFMA (gar_nnm_coord_mfma.hip); fp32 rows and
//               64 < n <= 128 here, from an LDS tile with mask-bit loops over the two mask words, as
//               k_bulyan_tail does, in plain IEEE sums (a non-finite member reaches exactly the sets
//               that hold it).
#include "gar_nnm_coord.hpp"
#include "gar_select.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

__global__ __launch_bounds__(1024) void k_nnm_sets(const float* __restrict__ gram, int np, int n, int c,
                                                   unsigned long long* __restrict__ masks) {
  extern __shared__ float lds_d[];   // n * (n + 1) distances, diagonal 0
  gram += static_cast<int64_t>(blockIdx.x) * np * np;
  masks += static_cast<int64_t>(blockIdx.x) * 2 * n;
  fill_distances(gram, np, n, lds_d, 0.f);
  __syncthreads();
  nnm_build_sets(lds_d, n, c, nullptr, masks);
}

// 128 x 129 fp32 distances = 64.5 KB at n = 128
static size_t nnm_sets_lds_bytes(int n) { return static_cast<size_t>(n) * (n + 1) * sizeof(float); }

void nnm_sets(const float* gram_in, int np, int n, int f, unsigned long long* masks, hipStream_t stream, int batch) {
  launch_select<k_nnm_sets>(batch, nnm_sets_lds_bytes(n), stream, gram_in, np, n, n - f, masks);
}

namespace coord {

namespace {

// tile width (coordinates, = threads per workgroup): the [NP x TW] tile stays within 32 KB
template <int DT, int NP>
constexpr int lds_tile_width() {
  constexpr int esz = (DT == kF32) ? 4 : 2;
  return 32768 / (NP * esz) < 256 ? 32768 / (NP * esz) : 256;
}

template <int DT, int NP, int MODE>
__global__ __launch_bounds__(256) void k_nnm_coord_lds(RowTable rows, int n, int64_t d, int f,
                                                       const u64* __restrict__ masks, void* out, int out_dt) {
  constexpr int ESZ = (DT == kF32) ? 4 : 2;
  constexpr int TW = lds_tile_width<DT, NP>();
  constexpr int CPR = TW * ESZ / 16;   // 16-byte chunks per tile row
  constexpr int WORDS = NP > 64 ? 2 : 1;
  __shared__ __align__(16) unsigned char tile[NP * TW * ESZ];
  __shared__ uint64_t smask[NP * WORDS];
  for (int e = threadIdx.x; e < NP * WORDS; e += blockDim.x) {
    const int k = e / WORDS, wd = e % WORDS;
    smask[e] = k < n ? static_cast<uint64_t>(masks[2 * k + wd]) : 0ull;
  }
  __syncthreads();
  const float inv_c = 1.f / static_cast<float>(n - f);
  const int64_t ntiles = d / TW;
  auto at = [&](int j, int col) -> float {
    if constexpr (DT == kF32) return reinterpret_cast<const float*>(tile)[j * TW + col];
    else return cvt16<DT>(reinterpret_cast<const uint16_t*>(tile)[j * TW + col]);
  };
  for (int64_t tb = blockIdx.x; tb < ntiles + 1; tb += gridDim.x) {
    const int64_t x0 = tb * TW;
    const int width = static_cast<int>(tb < ntiles ? TW : d - x0);   // last tile: the d % TW tail
    if (width <= 0) break;
    if (width == TW) {
      for (int ch = threadIdx.x; ch < n * CPR; ch += blockDim.x) {
        const int i = ch / CPR, k = ch % CPR;
        *reinterpret_cast<uint4*>(tile + (i * TW) * ESZ + k * 16) =
            *reinterpret_cast<const uint4*>(static_cast<const char*>(rows.p[i]) + x0 * ESZ + k * 16);
      }
    } else {
      for (int e = threadIdx.x; e < n * TW; e += blockDim.x) {   // columns >= width repeat column 0
        const int i = e / TW, k = e % TW;
        const int64_t xs = k < width ? x0 + k : x0;
        if constexpr (DT == kF32) reinterpret_cast<float*>(tile)[i * TW + k] = load_one<DT>(rows.p[i], xs);
        else reinterpret_cast<uint16_t*>(tile)[i * TW + k] = static_cast<const uint16_t*>(rows.p[i])[xs];
      }
    }
    __syncthreads();
    const int col = threadIdx.x;
    const int nn = opaque_uniform(n), ff = opaque_uniform(f);
    float v[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      v[k] = kInf;
      if (k < nn) {   // uniform; the masks are tile-invariant: volatile reads keep them out of registers
        float s = 0.f;
#pragma unroll
        for (int wd = 0; wd < WORDS; ++wd) {
          uint64_t m = uniform64(lds_volatile(smask[k * WORDS + wd]));
#pragma clang loop unroll(disable)
          while (m) {
            s += at(__builtin_ctzll(m) + 64 * wd, col);
            m &= m - 1;
          }
        }
        v[k] = s * inv_c;
      }
    }
    const float r = nnm_rule<NP, MODE>(v, nn, ff);
    if (col < width) store_one(out, out_dt, x0 + col, r);
    __syncthreads();
  }
}

template <int DT, int NP, int MODE>
void launch_lds(const RowTable& rows, int n, int64_t d, int f, const u64* masks, void* out, int out_dt, hipStream_t s) {
  constexpr int TW = lds_tile_width<DT, NP>();
  int64_t g = d / TW + 1;
  const int64_t cap = tail_grid_cap(4096);
  if (g > cap) g = cap;
  hipLaunchKernelGGL((k_nnm_coord_lds<DT, NP, MODE>), dim3(static_cast<unsigned>(g)), dim3(TW), 0, s, rows, n, d, f,
                     masks, out, out_dt);
}

template <int DT, int MODE>
void launch_lds_np(const RowTable& rows, int n, int64_t d, int f, const u64* masks, void* out, int out_dt,
                   hipStream_t s) {
  if constexpr (DT == kF32) {   // 16-bit rows with n <= 64 never come here
    if (n <= 8) return launch_lds<DT, 8, MODE>(rows, n, d, f, masks, out, out_dt, s);
    if (n <= 16) return launch_lds<DT, 16, MODE>(rows, n, d, f, masks, out, out_dt, s);
    if (n <= 32) return launch_lds<DT, 32, MODE>(rows, n, d, f, masks, out, out_dt, s);
    if (n <= 64) return launch_lds<DT, 64, MODE>(rows, n, d, f, masks, out, out_dt, s);
  }
  launch_lds<DT, 128, MODE>(rows, n, d, f, masks, out, out_dt, s);
}

template <int MODE>
void launch_mode(const RowTable& rows, int n, int64_t d, int dt, int f, const u64* masks, void* out, int out_dt,
                 hipStream_t s) {
  if (dt == kF32) launch_lds_np<kF32, MODE>(rows, n, d, f, masks, out, out_dt, s);
  else if (n <= 64) launch_nnm_coord_mfma(rows, n, d, dt, MODE, f, masks, out, out_dt, s);
  else if (dt == kBF16) launch_lds_np<kBF16, MODE>(rows, n, d, f, masks, out, out_dt, s);
  else launch_lds_np<kF16, MODE>(rows, n, d, f, masks, out, out_dt, s);
}

}  // namespace
}  // namespace coord

void nnm_coord(const RowTable& rows, int n, int64_t d, int dt, int mode, int f, const unsigned long long* masks,
               void* out, int out_dt, hipStream_t stream) {
  if (d <= 0) return;
  if (mode == kMedian) coord::launch_mode<kMedian>(rows, n, d, dt, f, masks, out, out_dt, stream);
  else coord::launch_mode<kTrimmedMean>(rows, n, d, dt, f, masks, out, out_dt, stream);
}

}  // namespace gpu
}  // namespace garfield

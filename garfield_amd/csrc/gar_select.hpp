// What the one-workgroup selections on the n x n Gram matrix share (Krum, Bulyan, geometric median,
// centered clipping, DnC, nearest-neighbour mixing; at the end, what the subset searches share): one
// 1024-thread workgroup (16 waves) per problem,
// the distances D in LDS with pitch n + 1, row i on wave i % 16, each lane owning columns
// (lane, lane + 64), n <= kMaxRows = 128. The validity policy of docs/GAR_SEMANTICS.md is written
// here once for the GPU (load_valid_distances, zero_infinite_distances) and once for the CPU
// (gar_cpu.cpp: valid_rows, Usable).
#pragma once
#include "gar_device.hpp"

namespace garfield {
namespace gpu {
namespace dev {

// Σ_{i < n} x[i] y[i] (y == nullptr: Σ x[i]) by one wave, n <= 128; identical on every wave
__device__ __forceinline__ double wave_dot(const double* x, const double* y, int n, int lane) {
  double acc = 0.0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int i = lane + 64 * c;
    if (i < n) acc += y ? x[i] * y[i] : x[i];
  }
  return wave_sum_f64(acc);
}

// v of the lane that the DPP control CTRL pairs with this one (all 64 lanes active)
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// Σ over the wave, the same bits in every lane, in a fixed pairing (DnC, CAF). A round is a chain of four
// dependent sums, so their latency is the kernel's time: the four steps inside a row of 16 lanes go
// through DPP (lane ^ 1, lane ^ 2, then the mirrored half rows and rows: both partners add the same
// two values) and only the two steps across rows through the LDS crossbar (wave_sum_f64 takes six).
__device__ __forceinline__ double wave_sum_dpp(double v) {
  v += dpp_f64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0x140>(v);   // row_mirror
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// Squared distances D (LDS, pitch n + 1) from a Gram matrix (pitch np) by the whole workgroup:
// non-finite -> +inf, clamped at 0, `diag` on the diagonal.
__device__ __forceinline__ void fill_distances(const float* __restrict__ gram, int np, int n, float* D,
                                               float diag = kInf) {
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e / n, j = e % n;
    float v;
    if (i == j) {
      v = diag;
    } else {
      v = gram[i * np + i] + gram[j * np + j] - 2.f * gram[i * np + j];
      if (!isfinite(v)) v = kInf;
      v = fmaxf(v, 0.f);
    }
    D[i * (n + 1) + j] = v;
  }
}

// The opening of the iterated selections: D with a zero diagonal, then valid[i] = row i has a finite
// off-diagonal distance (n flags), barriers included. Returns |V|, counted over the rows [0, nw).
// |V| == 0 (n == 1 or every pair non-finite) is the caller's plain-average branch.
__device__ __forceinline__ int load_valid_distances(const float* __restrict__ gram, int np, int n, int nw, float* D,
                                                    int* valid) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pitch = n + 1;
  fill_distances(gram, np, n, D, 0.f);
  __syncthreads();
  for (int i = wave; i < n; i += 16) {
    float cnt = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int j = lane + 64 * c;
      if (j < n && j != i && D[i * pitch + j] != kInf) cnt += 1.f;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) valid[i] = cnt > 0.f;
  }
  __syncthreads();
  int nv = 0;
  for (int i = 0; i < nw; ++i) nv += valid[i];
  return nv;
}

// An infinite distance between two valid rows (overflow) counts as 0. An invalid row's distances are
// all infinite, hence all zeroed: with a zero weight it adds exact zeros to every sum. No barrier:
// the caller's next one (after its vector init) publishes the sweep.
__device__ __forceinline__ void zero_infinite_distances(float* D, int n) {
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e / n, j = e % n;
    if (D[i * (n + 1) + j] == kInf) D[i * (n + 1) + j] = 0.f;
  }
}

// S_i = Σ_j A_j D_ij in fp64 (geometric median, centered clipping), reduced with wave_sum_f64. DnC's
// matvec pairs the lanes differently (another fp64 sum, other bits) and stays in gar_dnc.hip.
__device__ __forceinline__ void dist_matvec(const float* D, int n, const double* A, double* S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < n; i += 16) {
    const float* row = D + i * (n + 1);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int j = lane + 64 * c;
      if (j < n) acc += A[j] * static_cast<double>(row[j]);
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) S[i] = acc;
  }
}

// Krum score of row i (sum of the q smallest off-diagonal distances, +inf on the diagonal); also
// reports whether column j is among the q nearest. Ranks are counted, not sorted: rank(i,j) =
// #{k != i : (D_ik, k) < (D_ij, j)}, a strict total order.
__device__ __forceinline__ float row_score(const float* D, int n, int i, int q, int lane, bool keep[2]) {
  const float* row = D + i * (n + 1);
  float contrib = 0.f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int j = lane + 64 * c;
    keep[c] = false;
    if (j < n && j != i) {
      const float dj = row[j];
      int rank = 0;
      for (int k = 0; k < n; ++k) {
        const float dk = row[k];
        rank += (k != i) && (dk < dj || (dk == dj && k < j));
      }
      if (rank < q) { contrib += dj; keep[c] = true; }
    }
  }
  return wave_sum(contrib);
}

// The neighbour sets of nearest-neighbour mixing from the distances D of fill_distances (diagonal 0) by
// the whole workgroup: S_i = row i, then the c - 1 nearest others by (distance, index), as ranks
// counted by one lane per column and a ballot. Row i is wave i % (waves)'s; a set is two 64-bit mask
// words, written to `masks` and (when given) to the LDS copy Mk. Shared by k_nnm_mix and k_nnm_sets.
__device__ __forceinline__ void nnm_build_sets(const float* D, int n, int c, unsigned long long* Mk,
                                               unsigned long long* __restrict__ masks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int pitch = n + 1;
  for (int i = wave; i < n; i += nwaves) {
    const float* row = D + i * pitch;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int j = lane + 64 * cc;
      bool member = false;
      if (j < n) {
        if (j == i) {
          member = true;
        } else {
          const float dj = row[j];
          int rank = 0;
          for (int k = 0; k < n; ++k) {
            const float dk = row[k];
            rank += (k != i) && (dk < dj || (dk == dj && k < j));
          }
          member = rank < c - 1;
        }
      }
      const unsigned long long b = __ballot(member);
      if (lane == 0) {
        if (Mk) Mk[2 * i + cc] = b;
        masks[2 * i + cc] = b;
      }
    }
  }
}

// The subset searches (Brute, SMEA): the k-subsets of n rows as k-bit masks in increasing numeric order
// (combinatorial number system), rank = the position in that order.
__device__ __forceinline__ unsigned long long binom(int a, int b) {
  if (b < 0 || b > a) return 0ull;
  if (b > a - b) b = a - b;
  unsigned long long r = 1;
  for (int i = 1; i <= b; ++i) r = r * static_cast<unsigned long long>(a - b + i) / static_cast<unsigned long long>(i);
  return r;
}

// the mask of rank r
__device__ __forceinline__ unsigned long long subset_unrank(unsigned long long r, int n, int k) {
  unsigned long long mask = 0ull;
  int kk = k;
  for (int i = n - 1; i >= 0 && kk > 0; --i) {
    const unsigned long long c = binom(i, kk);
    if (c <= r) { mask |= 1ull << i; r -= c; --kk; }
  }
  return mask;
}

}  // namespace dev

// The searches reduce a (score bits << 32) | rank key with atomicMin: the key's start value, and the winner's
// weights 1 / k on its members (kScore: also the winning score, the key's high word, to *score).
// (a kernel defined in a header shared by two translation units: the dummy template parameter gives it the
// linkage of a template, one definition at link time)
template <int = 0> __global__ void k_subset_init(unsigned long long* best) { *best = ~0ull; }

template <bool kScore>
__global__ void k_subset_finalize(const unsigned long long* __restrict__ best, int n, int k,
                                  float* __restrict__ weights, float* __restrict__ score) {
  __shared__ unsigned long long mask;
  if (threadIdx.x == 0) {
    mask = dev::subset_unrank((*best) & 0xffffffffull, n, k);
    if (kScore) *score = __uint_as_float(static_cast<unsigned int>((*best) >> 32));
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < n) weights[i] = ((mask >> i) & 1ull) ? 1.f / static_cast<float>(k) : 0.f;
}

// Launch a selection kernel: `batch` workgroups of 1024 threads with lds_bytes of dynamic LDS. At
// n = 128 the distances alone are 64.5 KB, above the 64 KB default, so every kernel is opted in to
// 96 KB once (the attribute is a cap, the launch's size is what is allocated; a kernel's static
// __shared__ counts against the 160 KB too).
template <auto Kernel, class... A>
void launch_select(int batch, size_t lds_bytes, hipStream_t stream, A... args) {
  static const bool once = [] {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            96 * 1024) != hipSuccess)
      (void)hipGetLastError();  // never leave a sticky error for the framework to trip over
    return true;
  }();
  (void)once;
  hipLaunchKernelGGL(Kernel, dim3(batch), dim3(1024), lds_bytes, stream, args...);
}

}  // namespace gpu
}  // namespace garfield

// Nearest-neighbour mixing (NNM, Allouah et al., AISTATS 2023) on the Gram matrix.
//
// Before a rule runs, every gradient x_i is replaced by y_i = (1/c) Σ_{j∈S_i} x_j, the mean of its
// c = n - f nearest gradients (itself included). Mixing is linear, so nothing here touches the
// d-length rows: with D⁰ the squared distances with a zero diagonal and
//   M_ij = (1/c²) Σ_{k∈S_i} Σ_{l∈S_j} D⁰_kl,   ||y_i - y_j||² = M_ij - ½M_ii - ½M_jj
// (every row of the mixing matrix sums to 1). k_nnm_mix builds the sets and writes a pseudo-Gram H
// with H_ii = 0 and H_ij = -½ D'_ij, on which fill_distances yields 0 + 0 - 2H_ij = D'_ij exactly:
// the Krum and geometric-median selections run on H unchanged. k_nnm_unmix folds their weights a
// over the mixed rows back into weights over the original rows, w_j = (1/c) Σ_{i : j∈S_i} a_i, which
// the combine kernels consume. Semantics: docs/GAR_SEMANTICS.md "Nearest-neighbour mixing".
//
// Layout as in the Krum selection (gar_gram.hip): D in LDS with pitch n + 1, row i on wave i % 16,
// each lane owning columns (lane, lane + 64). A set is two 64-bit mask words (an arbitrary set per
// row: a later set builder can reuse everything after the ballot). All sums are fp64 over the set
// members in ascending index, the inner sum over l first: equal sets give bit-equal M, hence an
// exact zero distance, and the same Gram gives the same bits on every rank.
#include "gar_select.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

namespace {

typedef unsigned long long u64;

constexpr int kJB = 16;   // columns of R resident in LDS per pass (n x kJB fp64 = 16 KB at n = 128)

__device__ __forceinline__ bool in_set(u64 m0, u64 m1, int k) { return ((k < 64 ? m0 : m1) >> (k & 63)) & 1ull; }

// R[k][jj] = Σ_{l∈S_j} D⁰_kl for the columns j = j0 + jj of one pass (distances are >= 0 or +inf:
// a sum is +inf exactly when one of its terms is)
__device__ __forceinline__ void fill_R(const float* D, const u64* Mk, int n, int j0, double* R) {
  for (int e = threadIdx.x; e < n * kJB; e += blockDim.x) {
    const int k = e % n, jj = e / n, j = j0 + jj;
    double acc = 0.0;
    if (j < n) {
      const u64 m0 = Mk[2 * j], m1 = Mk[2 * j + 1];
      const float* row = D + k * (n + 1);
      for (int l = 0; l < n; ++l)
        if (in_set(m0, m1, l)) acc += static_cast<double>(row[l]);
    }
    R[k * kJB + jj] = acc;
  }
}

// M_ij for the resident column jj
__device__ __forceinline__ double set_sum(const double* R, const u64* Mk, int n, int c, int i, int jj) {
  const u64 m0 = Mk[2 * i], m1 = Mk[2 * i + 1];
  double acc = 0.0;
  for (int k = 0; k < n; ++k)
    if (in_set(m0, m1, k)) acc += R[k * kJB + jj];
  return acc / (static_cast<double>(c) * static_cast<double>(c));
}

}  // namespace

__global__ __launch_bounds__(1024) void k_nnm_mix(const float* __restrict__ gram, int np, int n, int c,
                                                  float* __restrict__ H, u64* __restrict__ masks) {
  extern __shared__ double lds64[];
  // workgroup b mixes problem b of a batch (one Gram per parameter segment)
  gram += static_cast<int64_t>(blockIdx.x) * np * np;
  H += static_cast<int64_t>(blockIdx.x) * np * np;
  masks += static_cast<int64_t>(blockIdx.x) * 2 * n;
  double* R = lds64;                                  // n * kJB
  double* Md = lds64 + n * kJB;                       // n   M_ii (+inf: row i is tainted)
  u64* Mk = reinterpret_cast<u64*>(Md + n);           // 2n  the sets
  float* D = reinterpret_cast<float*>(Mk + 2 * n);    // n * (n + 1), diagonal 0

  fill_distances(gram, np, n, D, 0.f);
  __syncthreads();
  // S_i: row i first, then the c - 1 nearest others by (distance, index); ranks are counted
  nnm_build_sets(D, n, c, Mk, masks);
  __syncthreads();
  // the M_ii first: R for kJB columns at a time, the fp64 n x n matrix does not fit next to D
  for (int j0 = 0; j0 < n; j0 += kJB) {
    fill_R(D, Mk, n, j0, R);
    __syncthreads();
    const int j = j0 + static_cast<int>(threadIdx.x);
    if (threadIdx.x < kJB && j < n) Md[j] = set_sum(R, Mk, n, c, j, threadIdx.x);
    __syncthreads();
  }
  // then every M_ij (i < j) streams into H, mirrored: H is exactly symmetric
  for (int j0 = 0; j0 < n; j0 += kJB) {
    fill_R(D, Mk, n, j0, R);
    __syncthreads();
    for (int e = threadIdx.x; e < n * kJB; e += blockDim.x) {
      const int jj = e % kJB, i = e / kJB, j = j0 + jj;
      if (j >= n || i > j) continue;
      if (i == j) {
        H[i * np + i] = 0.f;
        continue;
      }
      const double mij = set_sum(R, Mk, n, c, i, jj), mi = Md[i], mj = Md[j];
      float h = -kInf;   // a tainted row or an infinite cross pair
      if (!isinf(mij) && !isinf(mi) && !isinf(mj)) {
        const double v = fmax(mij - 0.5 * mi - 0.5 * mj, 0.0);
        h = v == 0.0 ? 0.f : -0.5f * static_cast<float>(v);
      }
      H[i * np + j] = h;
      H[j * np + i] = h;
    }
    __syncthreads();
  }
}

// w_j = (1/c) Σ_{i : j∈S_i} a_i / Σ_i a_i: i ascending in fp64, zero a_i skipped (a tainted row adds an
// exact zero). The fp32 a of a selection sum to 1 only within rounding; divided by their fp64 sum, w
// sums to 1 and equal sets (f = 0) give exactly 1/n.
__global__ __launch_bounds__(128) void k_nnm_unmix(const float* __restrict__ a, const u64* __restrict__ masks, int n,
                                                   int c, float* __restrict__ w) {
  a += static_cast<int64_t>(blockIdx.x) * n;
  masks += static_cast<int64_t>(blockIdx.x) * 2 * n;
  w += static_cast<int64_t>(blockIdx.x) * n;
  const int j = threadIdx.x;
  if (j >= n) return;
  double acc = 0.0, tot = 0.0;
  for (int i = 0; i < n; ++i) {
    const float ai = a[i];
    if (ai == 0.f) continue;
    tot += static_cast<double>(ai);
    if ((masks[2 * i + (j >> 6)] >> (j & 63)) & 1ull) acc += static_cast<double>(ai);
  }
  w[j] = tot == 0.0 ? 0.f : static_cast<float>(acc / tot / static_cast<double>(c));
}

// 128 x 129 fp32 distances + 128 x 16 fp64 R + sets and M_ii = 83.5 KB at n = 128
static size_t nnm_lds_bytes(int n) {
  return static_cast<size_t>(n * kJB + 3 * n) * sizeof(double) + static_cast<size_t>(n * (n + 1)) * sizeof(float);
}

void nnm_mix(const float* gram_in, int np, int n, int f, float* H, unsigned long long* masks, hipStream_t stream,
             int batch) {
  launch_select<k_nnm_mix>(batch, nnm_lds_bytes(n), stream, gram_in, np, n, n - f, H, masks);
}

void nnm_unmix(const float* a, const unsigned long long* masks, int n, int f, float* w, hipStream_t stream,
               int batch) {
  hipLaunchKernelGGL(k_nnm_unmix, dim3(batch), dim3(128), 0, stream, a, masks, n, n - f, w);
}

}  // namespace gpu
}  // namespace garfield

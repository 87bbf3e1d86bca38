// Geometric median (RFA / smoothed Weiszfeld) selection on the Gram matrix.
//
// The Weiszfeld iterate stays in the affine hull of the gradients, z = Σ_j a_j x_j with Σ a = 1,
// so its distance to every gradient follows from the pairwise squared distances D alone:
//   ||x_i - z||² = Σ_j a_j D_ij - ½ Σ_jk a_j a_k D_jk.
// The whole iteration therefore runs on the n x n matrix the split-K MFMA Gram kernel produces:
// one 1024-thread workgroup per problem, no pass over the d-length rows. The weights a feed the
// combine kernels unchanged. Semantics: docs/GAR_SEMANTICS.md "Geometric median".
//
// Layout as in the Krum selection (gar_gram.hip): D in LDS with pitch n + 1, row i on wave
// i % 16, each lane owning columns (lane, lane + 64). s, q and Σb are accumulated in fp64 (the
// matrix is tiny), the trip count is fixed and every reduction has a fixed shape: same Gram in,
// same bits out, on every rank.
#include "gar_device.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

__global__ __launch_bounds__(1024) void k_geomed_select(const float* __restrict__ gram, int np, int n, int iters,
                                                        double nu, float* __restrict__ weights,
                                                        float* __restrict__ dists) {
  extern __shared__ double lds64[];
  // workgroup b solves problem b of a batch (the layer-wise GAR: one Gram per parameter segment)
  gram += static_cast<int64_t>(blockIdx.x) * np * np;
  weights += static_cast<int64_t>(blockIdx.x) * n;
  dists += static_cast<int64_t>(blockIdx.x) * n;
  double* A = lds64;            // n weights a (0 on invalid rows)
  double* S = lds64 + n;        // n   s_i = Σ_j a_j D_ij
  double* B = lds64 + 2 * n;    // n   b_i = 1 / max(r_i, nu) (0 on invalid rows)
  float* D = reinterpret_cast<float*>(lds64 + 3 * n);   // n * (n + 1), diagonal 0
  int* valid = reinterpret_cast<int*>(D + n * (n + 1));  // n
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pitch = n + 1;

  fill_distances(gram, np, n, D, 0.f);   // the selections' distances, with a zero diagonal
  __syncthreads();
  // a row is valid when it has a finite off-diagonal distance
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
  for (int i = 0; i < n; ++i) nv += valid[i];
  const int me = threadIdx.x;
  if (nv == 0) {   // n == 1 or every pair non-finite: plain average (uniform branch)
    if (me < n) {
      weights[me] = 1.f / static_cast<float>(n);
      dists[me] = 0.f;
    }
    return;
  }
  // an infinite distance between two valid rows (overflow) counts as 0; invalid rows carry a = 0
  // and zeroed distances, so they add exact zeros to every sum
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e / n, j = e % n;
    if (D[i * pitch + j] == kInf) D[i * pitch + j] = 0.f;
  }
  if (me < n) {
    A[me] = valid[me] ? 1.0 / static_cast<double>(nv) : 0.0;
    S[me] = 0.0;
    B[me] = 0.0;
  }
  __syncthreads();
  double r = 0.0;
  for (int it = 0; it < iters; ++it) {
    for (int i = wave; i < n; i += 16) {
      const float* row = D + i * pitch;
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int j = lane + 64 * c;
        if (j < n) acc += A[j] * static_cast<double>(row[j]);
      }
      acc = wave_sum_f64(acc);
      if (lane == 0) S[i] = acc;
    }
    __syncthreads();
    const double q = 0.5 * wave_dot(A, S, n, lane);
    if (me < n && valid[me]) {
      r = sqrt(fmax(S[me] - q, 0.0));
      B[me] = 1.0 / fmax(r, nu);
    }
    __syncthreads();
    const double tot = wave_dot(B, nullptr, n, lane);
    if (me < n) A[me] = B[me] / tot;
    __syncthreads();
  }
  if (me < n) {
    weights[me] = static_cast<float>(A[me]);
    dists[me] = valid[me] ? static_cast<float>(r) : kInf;
  }
}

static size_t geomed_lds_bytes(int n) {
  return static_cast<size_t>(3 * n) * sizeof(double) + static_cast<size_t>(n * (n + 1) + n) * sizeof(float);
}

void geomed_select(const float* gram_in, int np, int n, int iters, double nu, float* weights, float* dists,
                   hipStream_t stream, int batch) {
  // 128 x 129 fp32 distances + 3 x 128 fp64 vectors = 69.6 KB > the 64 KB default: opt in to 96 KB
  static bool once = [] {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_geomed_select),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
      (void)hipGetLastError();  // never leave a sticky error for the framework to trip over
    return true;
  }();
  (void)once;
  hipLaunchKernelGGL(k_geomed_select, dim3(batch), dim3(1024), geomed_lds_bytes(n), stream, gram_in, np, n, iters, nu,
                     weights, dists);
}

}  // namespace gpu
}  // namespace garfield

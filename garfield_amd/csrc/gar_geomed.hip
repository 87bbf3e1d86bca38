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
#include "gar_select.hpp"

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
  const int lane = threadIdx.x & 63;

  const int nv = load_valid_distances(gram, np, n, n, D, valid);   // docs/GAR_SEMANTICS.md: the validity policy
  const int me = threadIdx.x;
  if (nv == 0) {   // n == 1 or every pair non-finite: plain average (uniform branch)
    if (me < n) {
      weights[me] = 1.f / static_cast<float>(n);
      dists[me] = 0.f;
    }
    return;
  }
  zero_infinite_distances(D, n);   // invalid rows carry a = 0 and zeroed distances: exact zeros in every sum
  if (me < n) {
    A[me] = valid[me] ? 1.0 / static_cast<double>(nv) : 0.0;
    S[me] = 0.0;
    B[me] = 0.0;
  }
  __syncthreads();
  double r = 0.0;
  for (int it = 0; it < iters; ++it) {
    dist_matvec(D, n, A, S);
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

// 128 x 129 fp32 distances + 3 x 128 fp64 vectors = 69.6 KB at n = 128
static size_t geomed_lds_bytes(int n) {
  return static_cast<size_t>(3 * n) * sizeof(double) + static_cast<size_t>(n * (n + 1) + n) * sizeof(float);
}

void geomed_select(const float* gram_in, int np, int n, int iters, double nu, float* weights, float* dists,
                   hipStream_t stream, int batch) {
  launch_select<k_geomed_select>(batch, geomed_lds_bytes(n), stream, gram_in, np, n, iters, nu, weights, dists);
}

}  // namespace gpu
}  // namespace garfield

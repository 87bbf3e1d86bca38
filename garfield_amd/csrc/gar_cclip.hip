// Centered clipping (Karimireddy, He, Jaggi, ICML 2021) selection on the Gram matrix.
//
// Each round moves the centre by at most tau: v <- v + (1/|V|) Σ_i (x_i - v) min(1, tau / ||x_i - v||).
// Started from an affine combination of the rows, the centre stays one, v = Σ_j a_j x_j with Σ a = 1,
// so its distance to every row follows from the pairwise squared distances D alone,
//   ||x_i - v||² = Σ_j a_j D_ij - ½ Σ_jk a_j a_k D_jk
// (the identity of the geometric median, gar_geomed.hip), and the update is a closed form on a:
//   a_j <- a_j (1 - Λ/|V|) + λ_j/|V|,   λ_i = min(1, tau / r_i),   Λ = Σ λ.
// The whole iteration runs on the n x n matrix of the split-K MFMA Gram kernel: one 1024-thread
// workgroup per problem, no pass over the d-length rows; the weights a feed the combine kernels
// unchanged. Rows nw..n-1 are basis-only (an appended centre vector): they may carry start weight
// but are never clipped or summed over. Semantics: docs/GAR_SEMANTICS.md "Centered clipping".
//
// Layout as in the Krum selection (gar_gram.hip): D in LDS with pitch n + 1, row i on wave i % 16,
// each lane owning columns (lane, lane + 64). All sums are fp64 in the fixed butterfly order of
// k_geomed_select, the trip count is fixed, the data-derived radius (the k-th smallest r) is found
// by rank counting: same Gram in, same bits out, on every rank. No atomics.
#include "gar_select.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

// a0 (nullable: uniform on the valid workers) may alias weights: thread i reads a0[i] before it
// writes weights[i] and touches no other entry.
__global__ __launch_bounds__(1024) void k_cclip_select(const float* __restrict__ gram, int np, int n, int nw,
                                                       const float* a0, double tau_in, int f, int iters,
                                                       float* weights, float* __restrict__ dists) {
  extern __shared__ double lds64[];
  // workgroup b solves problem b of a batch (the layer-wise GAR: one Gram per parameter segment)
  gram += static_cast<int64_t>(blockIdx.x) * np * np;
  weights += static_cast<int64_t>(blockIdx.x) * n;
  dists += static_cast<int64_t>(blockIdx.x) * n;
  if (a0) a0 += static_cast<int64_t>(blockIdx.x) * n;
  double* A = lds64;             // n weights a (0 on invalid rows)
  double* S = lds64 + n;         // n   s_i = Σ_j a_j D_ij
  double* R = lds64 + 2 * n;     // n   r_i on the valid workers
  double* Lm = lds64 + 3 * n;    // n   λ_i (0 off the valid workers)
  double* T = lds64 + 4 * n;     // 1   the data-derived radius
  float* D = reinterpret_cast<float*>(lds64 + 4 * n + 1);   // n * (n + 1), diagonal 0
  int* valid = reinterpret_cast<int*>(D + n * (n + 1));      // n
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  const int nv = load_valid_distances(gram, np, n, nw, D, valid);   // |V|: the valid workers
  const int me = threadIdx.x;
  if (nv == 0) {   // one worker or every pair non-finite: plain average of the workers
    if (me < n) {
      weights[me] = me < nw ? static_cast<float>(1.0 / static_cast<double>(nw)) : 0.f;
      dists[me] = 0.f;
    }
    return;
  }
  const double nvd = static_cast<double>(nv);
  const bool worker = me < nw && valid[me];
  const double uniform = worker ? 1.0 / nvd : 0.0;
  zero_infinite_distances(D, n);   // invalid rows carry a = 0 and zeroed distances: exact zeros in every sum
  if (me < n) {
    A[me] = a0 ? (valid[me] ? static_cast<double>(a0[me]) : 0.0) : uniform;
    S[me] = 0.0;
    R[me] = 0.0;
    Lm[me] = 0.0;
  }
  __syncthreads();
  if (a0) {   // the start divided by its sum; uniform on V when that sum is unusable
    const double tot = wave_dot(A, nullptr, n, lane);
    __syncthreads();
    if (me < n) A[me] = (isfinite(tot) && tot > 0.0) ? A[me] / tot : uniform;
    __syncthreads();
  }
  const int k = max(nv - f, 1);
  double r = 0.0;
  for (int it = 0; it < iters; ++it) {
    dist_matvec(D, n, A, S);
    __syncthreads();
    const double q = 0.5 * wave_dot(A, S, n, lane);
    if (worker) {
      r = sqrt(fmax(S[me] - q, 0.0));
      R[me] = r;
    }
    double tau = tau_in;
    if (!(tau_in > 0.0)) {   // the k-th smallest r over V by (value, index): ranks are counted,
      __syncthreads();       // one wave per row and a ballot over its two lane columns
      for (int i = wave; i < nw; i += 16) {
        if (!valid[i]) continue;
        const double ri = R[i];
        int rank = 0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int j = lane + 64 * c;
          bool before = false;
          if (j < nw && valid[j]) {
            const double rj = R[j];
            before = rj < ri || (rj == ri && j < i);
          }
          rank += __popcll(__ballot(before));
        }
        if (rank == k - 1 && lane == 0) T[0] = ri;
      }
      __syncthreads();
      tau = T[0];
    }
    if (worker) Lm[me] = r <= tau ? 1.0 : tau / r;
    __syncthreads();
    const double lam = wave_dot(Lm, nullptr, n, lane);
    if (me < n) A[me] = A[me] * (1.0 - lam / nvd) + Lm[me] / nvd;
    __syncthreads();
  }
  if (me < n) {
    weights[me] = static_cast<float>(A[me]);
    dists[me] = worker ? static_cast<float>(r) : kInf;
  }
}

// 128 x 129 fp32 distances + 4 x 128 fp64 vectors = 70.6 KB at n = 128
static size_t cclip_lds_bytes(int n) {
  return static_cast<size_t>(4 * n + 1) * sizeof(double) + static_cast<size_t>(n * (n + 1) + n) * sizeof(float);
}

void cclip_select(const float* gram_in, int np, int n, int nw, const float* a0, double tau, int f, int iters,
                  float* weights, float* dists, hipStream_t stream, int batch) {
  launch_select<k_cclip_select>(batch, cclip_lds_bytes(n), stream, gram_in, np, n, nw, a0, tau, f, iters, weights,
                                dists);
}

}  // namespace gpu
}  // namespace garfield

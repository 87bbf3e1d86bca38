// DnC spectral filtering (Shejwalkar & Houmansadr, NDSS 2021) selection on the Gram matrix.
//
// With the rows centred at their mean, C = X - 1μᵀ, classical MDS gives C Cᵀ = K = -½ J D J with
// J = I - 11ᵀ/n and D the pairwise squared distances. If (λ, u) is the top eigenpair of K, the top
// right singular vector of C is v = Cᵀu/√λ and the paper's outlier score of row i, its squared
// projection on v, is λ u_i². A power iteration on the n x n matrix of the split-K MFMA Gram kernel
// therefore gives the exact scores over all d coordinates: one 1024-thread workgroup per problem,
// no SVD, no pass over the d-length rows, no coordinate sub-sampling. K is never stored: K b is
// "centre b, multiply by D, centre, halve and negate". The weights (1 / kv on the kv lowest scores)
// feed the combine kernels unchanged. Semantics: docs/GAR_SEMANTICS.md "Spectral filtering".
//
// Layout as in the Krum selection (gar_gram.hip): D in LDS with pitch n + 1, row i on wave i % 16,
// each lane owning columns (lane, lane + 64). A round is one matvec phase, t = D (u - mean u), and
// one phase of means, norm and update, which every wave runs redundantly on the lane-owned columns
// of t in registers (three fp64 wave sums): t is double-buffered, so a round costs one barrier.
// All sums are fp64 in a fixed pairing of the lanes and the trip count is fixed: same Gram in, same
// bits out, on every rank. No atomics.
#include "gar_select.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

__global__ __launch_bounds__(1024) void k_dnc_select(const float* __restrict__ gram, int np, int n, int m, int iters,
                                                     float* __restrict__ weights, float* __restrict__ scores) {
  extern __shared__ double lds64[];
  // workgroup b solves problem b of a batch (the layer-wise GAR: one Gram per parameter segment)
  gram += static_cast<int64_t>(blockIdx.x) * np * np;
  weights += static_cast<int64_t>(blockIdx.x) * n;
  scores += static_cast<int64_t>(blockIdx.x) * n;
  double* R = lds64;             // n   r_i = mean_V D_ij (0 on invalid rows)
  double* T0 = lds64 + n;        // n   t of the even rounds
  double* T1 = lds64 + 2 * n;    // n   t of the odd rounds
  float* D = reinterpret_cast<float*>(lds64 + 3 * n);   // n * (n + 1), diagonal 0
  float* Sc = D + n * (n + 1);                          // n fp32 scores (+inf on invalid rows)
  int* valid = reinterpret_cast<int*>(Sc + n);          // n
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pitch = n + 1;

  const int nv = load_valid_distances(gram, np, n, n, D, valid);   // docs/GAR_SEMANTICS.md: the validity policy
  const int me = threadIdx.x;
  if (nv == 0) {   // n == 1 or every pair non-finite: plain average (uniform branch)
    if (me < n) {
      weights[me] = static_cast<float>(1.0 / static_cast<double>(n));
      scores[me] = 0.f;
    }
    return;
  }
  const double nvd = static_cast<double>(nv);
  const int kv = min(m, nv);   // non-finite rows use up the removal budget first
  zero_infinite_distances(D, n);   // an invalid row's distances are all zeroed: exact zeros in every sum
  __syncthreads();
  for (int i = wave; i < n; i += 16) {
    const float* row = D + i * pitch;
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int j = lane + 64 * c;
      if (j < n) acc += static_cast<double>(row[j]);
    }
    acc = wave_sum_dpp(acc);
    if (lane == 0) R[i] = acc / nvd;
  }
  __syncthreads();
  // From here on every wave holds, for its lanes' two columns, the same values as every other wave.
  const int j0 = lane, j1 = lane + 64;
  const bool v0 = j0 < n && valid[j0], v1 = j1 < n && valid[j1];
  const double r0 = v0 ? R[j0] : 0.0, r1 = v1 ? R[j1] : 0.0;
  const double g = wave_sum_dpp(r0 + r1) / nvd;
  // i*: the lowest valid index that attains max κ, κ_i = r_i - g/2 (the row farthest from the mean)
  double kb = -static_cast<double>(kInf);
  int star = n;
  if (v0) { kb = r0 - 0.5 * g; star = j0; }
  if (v1 && r1 - 0.5 * g > kb) { kb = r1 - 0.5 * g; star = j1; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ko = __shfl_xor(kb, o, 64);
    const int so = __shfl_xor(star, o, 64);
    if (ko > kb || (ko == kb && so < star)) { kb = ko; star = so; }
  }
  // the start: column i* of K (K·1 = 0, so a uniform start is useless)
  const double rs = R[star];
  double b0 = v0 ? -0.5 * (static_cast<double>(D[j0 * pitch + star]) - r0 - rs + g) : 0.0;
  double b1 = v1 ? -0.5 * (static_cast<double>(D[j1 * pitch + star]) - r1 - rs + g) : 0.0;
  double u0 = 0.0, u1 = 0.0;
  double* Tw = T0;   // written by this round's matvec
  double* Tr = T1;   // read by the next round
  for (int it = 0; it < iters; ++it) {
    // means, norm and update on the lane-owned columns
    const double nu = sqrt(wave_sum_dpp(b0 * b0 + b1 * b1));
    u0 = nu > 0.0 ? b0 / nu : 0.0;
    u1 = nu > 0.0 ? b1 / nu : 0.0;
    const double c = wave_sum_dpp(u0 + u1) / nvd;
    const double c0 = v0 ? u0 - c : 0.0, c1 = v1 ? u1 - c : 0.0;
    // matvec: t_i = Σ_j D_ij (u_j - c)
    for (int i = wave; i < n; i += 16) {
      const float* row = D + i * pitch;
      double acc = c0 * static_cast<double>(row[j0 < n ? j0 : 0]);   // c0 == 0 when j0 >= n
      if (j1 < n) acc += c1 * static_cast<double>(row[j1]);
      acc = wave_sum_dpp(acc);
      if (lane == 0) Tw[i] = acc;
    }
    __syncthreads();
    double* tmp = Tw; Tw = Tr; Tr = tmp;
    const double t0 = v0 ? Tr[j0] : 0.0, t1 = v1 ? Tr[j1] : 0.0;
    const double tm = wave_sum_dpp(t0 + t1) / nvd;
    b0 = v0 ? -0.5 * (t0 - tm) : 0.0;
    b1 = v1 ? -0.5 * (t1 - tm) : 0.0;
  }
  // λ = uᵀ K u; score_i = (K u)_i² / λ = λ u_i² at convergence
  const double lam = wave_sum_dpp(u0 * b0 + u1 * b1);
  if (wave == 0) {
    if (j0 < n) Sc[j0] = v0 ? (lam > 0.0 ? static_cast<float>(b0 * b0 / lam) : 0.f) : kInf;
    if (j1 < n) Sc[j1] = v1 ? (lam > 0.0 ? static_cast<float>(b1 * b1 / lam) : 0.f) : kInf;
  }
  __syncthreads();
  if (me < n) {
    // invalid rows carry +inf and rank after every valid row; kv <= nv keeps them out
    const bool keep = valid[me] && score_rank(Sc, n, me) < kv;
    weights[me] = keep ? static_cast<float>(1.0 / static_cast<double>(kv)) : 0.f;
    scores[me] = Sc[me];
  }
}

// 128 x 129 fp32 distances + 3 x 128 fp64 vectors + scores and flags = 69.1 KB at n = 128
static size_t dnc_lds_bytes(int n) {
  return static_cast<size_t>(3 * n) * sizeof(double) + static_cast<size_t>(n * (n + 1) + 2 * n) * sizeof(float);
}

void dnc_select(const float* gram_in, int np, int n, int m, int iters, float* weights, float* scores,
                hipStream_t stream, int batch) {
  launch_select<k_dnc_select>(batch, dnc_lds_bytes(n), stream, gram_in, np, n, m, iters, weights, scores);
}

}  // namespace gpu
}  // namespace garfield

// CAF, the covariance-bound agnostic filter (Allouah, Guerraoui, Gupta, Pinot, Rizk, Voitovych), on the
// Gram matrix.
//
// With weights a (Σa = 1) and μ_a = Σ a_i x_i, K_ij = (x_i - μ_a)·(x_j - μ_a) follows from the squared
// distances alone: ‖x_i - μ_a‖² = s_i - q/2 with s = D a, q = a·s, and
// K p = -½ (D p - s Σp - (s·p) 1 + q Σp 1). The n x n matrix M = A^½ K A^½ has the non-zero eigenvalues
// of the d x d weighted covariance Σ_i a_i (x_i - μ_a)(x_i - μ_a)ᵀ, and for its top eigenpair (λ, u) the
// squared projection of x_i - μ_a on the covariance's top eigenvector is τ_i = (K A^½ u)_i² / λ. A pass is
// therefore one s = D a matvec, a start (column i* of M, read from D) and `iters` power rounds on the
// n x n matrix of the split-K MFMA Gram kernel; then every row that still carries weight is scaled by
// 1 - τ_i / τ_max, and the weights of the pass of smallest λ are kept. No pass over the d-length rows.
// Semantics: docs/GAR_SEMANTICS.md "Covariance filter".
//
// Layout as in the DnC selection (gar_dnc.hip): D in LDS with pitch n + 1, row i on wave i % 16, each lane
// owning columns (lane, lane + 64). The vectors c, a, √a, s, u, b and the best a live in registers on the
// lane-owned columns, the same values in every wave; only the matvec's result goes through LDS, double-
// buffered, so a power round costs one barrier. Whether another pass runs is decided by thread 0 alone,
// written to LDS and read by every thread after a barrier: no barrier is reached by part of the workgroup.
// All sums are fp64 in a fixed pairing of the lanes: same Gram in, same bits out. No atomics.
#include "gar_select.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

// (max v, the lowest index that attains it) over the wave, the same in every lane
__device__ __forceinline__ void wave_argmax_f64(double& v, int& idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double vo = __shfl_xor(v, o, 64);
    const int io = __shfl_xor(idx, o, 64);
    if (vo > v || (vo == v && io < idx)) { v = vo; idx = io; }
  }
}

// T_i = Σ_j D_ij p_j for the lane-owned p (p0 == 0 on the lanes with lane >= n), row i on wave i % 16
__device__ __forceinline__ void caf_matvec(const float* D, int n, double p0, double p1, double* T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = lane, j1 = lane + 64;
  for (int i = wave; i < n; i += 16) {
    const float* row = D + i * (n + 1);
    double acc = p0 * static_cast<double>(row[j0 < n ? j0 : 0]);
    if (j1 < n) acc += p1 * static_cast<double>(row[j1]);
    acc = wave_sum_dpp(acc);
    if (lane == 0) T[i] = acc;
  }
}

__global__ __launch_bounds__(1024) void k_caf_select(const float* __restrict__ gram, int np, int n, int f, int iters,
                                                     int max_passes, float* __restrict__ weights,
                                                     float* __restrict__ lams) {
  extern __shared__ double lds64[];
  // workgroup b solves problem b of a batch (the layer-wise GAR: one Gram per parameter segment)
  gram += static_cast<int64_t>(blockIdx.x) * np * np;
  weights += static_cast<int64_t>(blockIdx.x) * n;
  lams += static_cast<int64_t>(blockIdx.x) * n;
  double* T0 = lds64;        // n   the matvec's result of the even rounds
  double* T1 = lds64 + n;    // n   and of the odd rounds
  float* D = reinterpret_cast<float*>(lds64 + 2 * n);   // n * (n + 1), diagonal 0
  float* Lm = D + n * (n + 1);                          // n   λ per pass (+inf beyond the last)
  int* valid = reinterpret_cast<int*>(Lm + n);          // n
  int* go = valid + n;                                  // 2   "run pass p" at p % 2
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pitch = n + 1;
  const int me = threadIdx.x;

  if (me < n) Lm[me] = kInf;
  const int nv = load_valid_distances(gram, np, n, n, D, valid);   // docs/GAR_SEMANTICS.md: the validity policy
  if (nv == 0) {   // n == 1 or every pair non-finite: plain average (uniform branch)
    if (me < n) {
      weights[me] = static_cast<float>(1.0 / static_cast<double>(n));
      lams[me] = kInf;
    }
    return;
  }
  zero_infinite_distances(D, n);   // published by the first pass's barrier
  // From here on every wave holds, for its lanes' two columns, the same values as every other wave.
  const int j0 = lane, j1 = lane + 64;
  const bool v0 = j0 < n && valid[j0], v1 = j1 < n && valid[j1];
  double c0 = v0 ? 1.0 : 0.0, c1 = v1 ? 1.0 : 0.0;   // invalid rows use up the removal budget first
  double sc = wave_sum_dpp(c0 + c1);
  double ba0 = c0 / sc, ba1 = c1 / sc;   // the a of the pass of smallest λ
  double best = static_cast<double>(kInf);
  const double keep_above = static_cast<double>(n) - 2.0 * static_cast<double>(f);
  const int maxp = (max_passes <= 0 || max_passes > n) ? n : max_passes;
  bool stop = false;
  double* Tw = T0;   // written by the next matvec
  double* Tr = T1;   // read after its barrier
  for (int pass = 0; pass < maxp; ++pass) {
    if (me == 0) go[pass & 1] = !stop && sc > keep_above;
    __syncthreads();
    if (!go[pass & 1]) break;
    const double a0 = c0 / sc, a1 = c1 / sc;
    const double ra0 = sqrt(a0), ra1 = sqrt(a1);
    caf_matvec(D, n, a0, a1, Tw);
    __syncthreads();
    { double* tmp = Tw; Tw = Tr; Tr = tmp; }
    const double s0 = v0 ? Tr[j0] : 0.0, s1 = v1 ? Tr[j1] : 0.0;
    const double q = wave_sum_dpp(a0 * s0 + a1 * s1);
    // i*: the lowest index that attains max a_i ‖x_i - μ_a‖²
    double vb = -static_cast<double>(kInf);
    int star = n;
    if (j0 < n) { vb = a0 * (s0 - 0.5 * q); star = j0; }
    if (j1 < n && a1 * (s1 - 0.5 * q) > vb) { vb = a1 * (s1 - 0.5 * q); star = j1; }
    wave_argmax_f64(vb, star);
    // the start: column i* of M, K(√a_{i*} e_{i*}) from column i* of D
    const double ras = __shfl(star < 64 ? ra0 : ra1, star & 63, 64);
    const double ss = __shfl(star < 64 ? s0 : s1, star & 63, 64);
    double kp0 = v0 ? -0.5 * (ras * static_cast<double>(D[j0 * pitch + star]) - s0 * ras - ss * ras + q * ras) : 0.0;
    double kp1 = v1 ? -0.5 * (ras * static_cast<double>(D[j1 * pitch + star]) - s1 * ras - ss * ras + q * ras) : 0.0;
    double b0 = ra0 * kp0, b1 = ra1 * kp1;
    double u0 = 0.0, u1 = 0.0;
    for (int it = 0; it < iters; ++it) {
      const double nb = sqrt(wave_sum_dpp(b0 * b0 + b1 * b1));
      u0 = nb > 0.0 ? b0 / nb : 0.0;
      u1 = nb > 0.0 ? b1 / nb : 0.0;
      const double p0 = ra0 * u0, p1 = ra1 * u1;
      const double sp = wave_sum_dpp(p0 + p1);
      const double sdp = wave_sum_dpp(s0 * p0 + s1 * p1);
      caf_matvec(D, n, p0, p1, Tw);
      __syncthreads();
      { double* tmp = Tw; Tw = Tr; Tr = tmp; }
      kp0 = v0 ? -0.5 * (Tr[j0] - s0 * sp - sdp + q * sp) : 0.0;
      kp1 = v1 ? -0.5 * (Tr[j1] - s1 * sp - sdp + q * sp) : 0.0;
      b0 = ra0 * kp0;
      b1 = ra1 * kp1;
    }
    // λ = uᵀ M u; τ_i = (K A^½ u)_i² / λ
    const double lam = wave_sum_dpp(u0 * b0 + u1 * b1);
    const double tau0 = lam > 0.0 ? kp0 * kp0 / lam : 0.0, tau1 = lam > 0.0 ? kp1 * kp1 / lam : 0.0;
    if (lam < best) {   // strict: the first pass wins a tie
      best = lam;
      ba0 = a0;
      ba1 = a1;
    }
    if (me == 0) Lm[pass] = static_cast<float>(lam);
    // τmax over the rows that still carry weight: its row gets an exact zero
    double tm = fmax(c0 > 0.0 ? tau0 : 0.0, c1 > 0.0 ? tau1 : 0.0);
    int unused = 0;
    wave_argmax_f64(tm, unused);
    if (lam > 0.0 && tm > 0.0) {
      if (c0 > 0.0) c0 *= 1.0 - fmin(tau0 / tm, 1.0);
      if (c1 > 0.0) c1 *= 1.0 - fmin(tau1 / tm, 1.0);
      sc = wave_sum_dpp(c0 + c1);
    } else {
      stop = true;
    }
  }
  __syncthreads();   // the last pass's λ
  if (wave == 0) {
    if (j0 < n) weights[j0] = static_cast<float>(ba0);
    if (j1 < n) weights[j1] = static_cast<float>(ba1);
  }
  if (me < n) lams[me] = Lm[me];
}

// 128 x 129 fp32 distances + 2 x 128 fp64 vectors + λ per pass, flags and the loop decision = 67.5 KB at n = 128
static size_t caf_lds_bytes(int n) {
  return static_cast<size_t>(2 * n) * sizeof(double) + static_cast<size_t>(n * (n + 1) + 2 * n + 2) * sizeof(float);
}

void caf_select(const float* gram_in, int np, int n, int f, int iters, int max_passes, float* weights, float* lams,
                hipStream_t stream, int batch) {
  launch_select<k_caf_select>(batch, caf_lds_bytes(n), stream, gram_in, np, n, f, iters, max_passes, weights, lams);
}

}  // namespace gpu
}  // namespace garfield

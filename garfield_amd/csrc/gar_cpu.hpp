// CPU implementations of every aggregation rule (float / double), used by the
// gloo / CPU configuration and as a second, independent implementation for the
// GPU kernels' tests. Semantics (tie-breaking, non-finite policy) are the ones
// documented in docs/GAR_SEMANTICS.md and are shared with the HIP kernels.
//
// Reference counterparts: py_krum/krum.cpp:50-118, py_bulyan/bulyan.cpp:53-193,
// py_median/median.cpp:42-77, py_brute/brute.cpp:47-113,
// TF deprecated_native/native.cpp:714-782 (averaged-median, average-nan).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace garfield {
namespace cpu {

template <class T>
struct Rows {
  std::vector<const T*> p;
  size_t n = 0;
  size_t d = 0;
};

// D[i*n + j] = ||g_i - g_j||^2 (double accumulation, fixed chunk order);
// non-finite -> +inf, diagonal -> +inf.
template <class T> std::vector<double> pairwise_sqdist(const Rows<T>& r);

// Selections (operate on the distance matrix, n x n).
std::vector<float> krum_weights(const std::vector<double>& D, size_t n, size_t f, size_t m,
                                std::vector<double>* scores = nullptr);
std::vector<float> bulyan_weights(const std::vector<double>& D, size_t n, size_t f, size_t m, size_t t);
std::vector<float> brute_weights(const std::vector<double>& D, size_t n, size_t f);
// SMEA (docs/GAR_SEMANTICS.md): among the C(n, n - f) subsets in Brute's order (n <= 64), 1 / (n - f) on the
// members of the one whose covariance has the smallest top eigenvalue λ (`iters` power rounds on the subset's
// block of D, fp32, ties to the lowest rank; +inf with a non-finite pair); *lam = the winning λ.
std::vector<float> smea_weights(const std::vector<double>& D, size_t n, size_t f, size_t iters,
                                float* lam = nullptr);
std::vector<float> aksel_weights(const std::vector<double>& dists, size_t n, size_t c);
// Geometric median (smoothed Weiszfeld, `iters` rounds on D alone): rows without a finite
// off-diagonal distance get weight 0; none valid -> uniform 1/n.
std::vector<float> geomed_weights(const std::vector<double>& D, size_t n, size_t iters, double nu);
// Centered clipping (`iters` rounds on D alone; docs/GAR_SEMANTICS.md): rows 0..nw-1 are the workers,
// rows nw..n-1 basis-only; a0 (empty: uniform on the workers) the start weights; tau > 0 the radius,
// tau <= 0 the max(|V| - f, 1)-th smallest distance of the centre to a valid worker, every round.
std::vector<float> cclip_weights(const std::vector<double>& D, size_t n, size_t nw, const std::vector<double>& a0,
                                 double tau, size_t f, size_t iters);

// DnC spectral filtering (`iters` power rounds on K = -½ J D J, from D alone): weight 1 / kv on the
// kv = min(m, |V|) valid rows of lowest (fp32 score, index), 0 elsewhere; scores[n] = λ u_i², +inf on
// rows without a finite off-diagonal distance; none valid -> uniform 1/n and zero scores.
std::vector<float> dnc_weights(const std::vector<double>& D, size_t n, size_t m, size_t iters,
                               std::vector<float>* scores = nullptr);

// CAF covariance filter (from D alone; docs/GAR_SEMANTICS.md): while more than n - 2f rows' worth of weight
// is left (at most max_passes passes, 0 = n), `iters` power rounds give the top eigenpair of the weighted
// covariance and every row is down-weighted by its squared projection on it; the weights of the pass of
// smallest λ are returned. lams[n] = λ of pass p at index p, +inf beyond the last pass; rows without a finite
// off-diagonal distance get weight 0 and use up the budget; none valid -> uniform 1/n.
std::vector<float> caf_weights(const std::vector<double>& D, size_t n, size_t f, size_t iters, size_t max_passes,
                               std::vector<float>* lams = nullptr);

// Nearest-neighbour mixing on D alone (0 <= f < n, c = n - f; docs/GAR_SEMANTICS.md). nnm_mix: masks[2n]
// (row i's set, i and its c - 1 nearest, as two 64-bit words; n <= 128) and the squared distances D' of
// the mixed rows (+inf diagonal), for the selections above. nnm_unmix: the selection's weights a over
// the mixed rows folded back onto the original rows.
std::vector<double> nnm_mix(const std::vector<double>& D, size_t n, size_t f, std::vector<uint64_t>* masks);
std::vector<float> nnm_unmix(const std::vector<float>& a, const std::vector<uint64_t>& masks, size_t n, size_t c);

// nnm_sets: the masks of nnm_mix alone. mixed_coordwise: NNM before a coordinate-wise rule, out[x] =
// the rule (mode kTrimmedMean with f, or kMedian) over the n set means (1/c) Σ_{j∈S_i} row_j[x] of the
// sets in `masks` (fp64 sums, members ascending); the mixed rows are never stored.
std::vector<uint64_t> nnm_sets(const std::vector<double>& D, size_t n, size_t f);
template <class T>
void mixed_coordwise(const Rows<T>& r, const std::vector<uint64_t>& masks, size_t c, int mode, size_t f, T* out);

// out = Σ_j w[j] g_j (accumulated in double)
template <class T> void combine(const Rows<T>& r, const std::vector<float>& w, T* out);

// Coordinate-wise rule (mode: garfield::CoordMode); W/t only for kBulyanTail.
template <class T>
void coordwise(const Rows<T>& r, int mode, size_t f, size_t beta, const std::vector<float>& W, size_t t,
               uint64_t seed, uint64_t threshold, T* out);

// dist_j = ||g_j - center||^2
template <class T> std::vector<double> sqdist_to(const Rows<T>& r, const T* center);

// Worker-side momentum in place on coordinates [lo, hi) of k rows (docs/GAR_SEMANTICS.md): X row r at
// X + r * xstride elements of dtype dt (garfield::DType: f32 / bf16 / f16), the fp32 state M row r at
// M + r * ld. First step: m <- g; later: m <- fmaf(beta, m, omega * g); then row <- the state rounded
// to nearest even. A non-finite g stays in the row and leaves m unchanged. Fixed chunking; the same
// formula as the HIP kernel (worker_mom.hip): equal inputs give equal bits.
void worker_momentum(void* X, int dt, int64_t xstride, float* M, int64_t ld, size_t k, size_t lo, size_t hi, float beta,
                     float omega, bool first);

}  // namespace cpu
}  // namespace garfield

#include "gar_cpu.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <mutex>
#include <numeric>
#include <stdexcept>

#include "gar_common.hpp"
#include "threadpool.hpp"

namespace garfield {
namespace cpu {

namespace {

constexpr double kInf = std::numeric_limits<double>::infinity();

inline double nan_to_inf(double v) { return v == v ? v : kInf; }

// Strict total order (value with NaN as +inf, index): the order every rank and
// every backend uses, so selections are identical everywhere.
inline bool key_less(double a, size_t ia, double b, size_t ib) {
  a = nan_to_inf(a);
  b = nan_to_inf(b);
  return a < b || (a == b && ia < ib);
}

}  // namespace

template <class T>
std::vector<double> pairwise_sqdist(const Rows<T>& r) {
  const size_t n = r.n, d = r.d;
  const size_t npairs = n * (n - 1) / 2;
  const size_t nchunks = default_chunks(d);
  std::vector<double> partial(nchunks * npairs, 0.0);
  parallel_for(0, d, nchunks, [&](size_t c, size_t lo, size_t hi) {
    double* out = partial.data() + c * npairs;
    size_t k = 0;
    for (size_t i = 0; i + 1 < n; ++i) {
      const T* a = r.p[i];
      for (size_t j = i + 1; j < n; ++j, ++k) {
        const T* b = r.p[j];
        double s = 0.0;
        for (size_t x = lo; x < hi; ++x) {
          const double v = static_cast<double>(a[x]) - static_cast<double>(b[x]);
          s += v * v;
        }
        out[k] = s;
      }
    }
  });
  std::vector<double> D(n * n, kInf);
  size_t k = 0;
  for (size_t i = 0; i + 1 < n; ++i) {
    for (size_t j = i + 1; j < n; ++j, ++k) {
      double s = 0.0;
      for (size_t c = 0; c < nchunks; ++c) s += partial[c * npairs + k];
      if (!std::isfinite(s)) s = kInf;
      D[i * n + j] = s;
      D[j * n + i] = s;
    }
  }
  return D;
}

// Per-row nearest set: ids of the q smallest off-diagonal distances by (D, j).
static std::vector<size_t> nearest(const std::vector<double>& D, size_t n, size_t i, size_t q) {
  std::vector<size_t> ids;
  ids.reserve(n - 1);
  for (size_t j = 0; j < n; ++j)
    if (j != i) ids.push_back(j);
  std::sort(ids.begin(), ids.end(),
            [&](size_t a, size_t b) { return key_less(D[i * n + a], a, D[i * n + b], b); });
  if (ids.size() > q) ids.resize(q);
  return ids;
}

static std::vector<size_t> rank_order(const std::vector<double>& s) {
  std::vector<size_t> order(s.size());
  std::iota(order.begin(), order.end(), size_t{0});
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return key_less(s[a], a, s[b], b); });
  return order;
}

std::vector<float> krum_weights(const std::vector<double>& D, size_t n, size_t f, size_t m,
                                std::vector<double>* scores_out) {
  if (n < 2 * f + 3) throw std::invalid_argument("krum: n must be >= 2f + 3");
  const size_t q = n - f - 2;
  std::vector<double> scores(n, 0.0);
  for (size_t i = 0; i < n; ++i) {
    double s = 0.0;
    for (size_t j : nearest(D, n, i, q)) s += D[i * n + j];
    scores[i] = s;
  }
  const auto order = rank_order(scores);
  std::vector<float> w(n, 0.f);
  for (size_t r = 0; r < m && r < n; ++r) w[order[r]] = 1.f / static_cast<float>(m);
  if (scores_out) *scores_out = scores;
  return w;
}

// The validity policy of the iterated selections (docs/GAR_SEMANTICS.md "Geometric median"; on the GPU:
// gar_select.hpp). valid[i]: row i has a finite off-diagonal distance; nv = |V|, counted over the rows [0, nw).
struct ValidRows {
  std::vector<char> valid;
  size_t nv = 0;
};
static ValidRows valid_rows(const std::vector<double>& D, size_t n, size_t nw) {
  ValidRows v{std::vector<char>(n, 0), 0};
  for (size_t i = 0; i < n; ++i) {
    for (size_t j = 0; j < n; ++j)
      if (j != i && std::isfinite(D[i * n + j])) v.valid[i] = 1;
    if (i < nw) v.nv += v.valid[i];
  }
  return v;
}

// The usable distance: the diagonal and an infinite distance between two valid rows count as 0.
struct Usable {
  const std::vector<double>& D;
  size_t n;
  double operator()(size_t i, size_t j) const {
    const double v = D[i * n + j];
    return (i != j && std::isfinite(v)) ? v : 0.0;
  }
};

// s = D a over the valid rows, in index order; returns q = ½ aᵀ s (geometric median, centered clipping).
static double dist_quadratic(const Usable& dist, const std::vector<char>& valid, const std::vector<double>& a,
                             std::vector<double>& s) {
  const size_t n = a.size();
  for (size_t i = 0; i < n; ++i) {
    if (!valid[i]) continue;
    double acc = 0.0;
    for (size_t j = 0; j < n; ++j)
      if (valid[j]) acc += a[j] * dist(i, j);
    s[i] = acc;
  }
  double q = 0.0;
  for (size_t i = 0; i < n; ++i)
    if (valid[i]) q += a[i] * s[i];
  return 0.5 * q;
}

// Smoothed Weiszfeld on the distance matrix alone (docs/GAR_SEMANTICS.md "Geometric median"):
// exactly `iters` rounds, every sum in index order over the valid rows.
std::vector<float> geomed_weights(const std::vector<double>& D, size_t n, size_t iters, double nu) {
  const auto [valid, nv] = valid_rows(D, n, n);
  if (nv == 0) return std::vector<float>(n, 1.f / static_cast<float>(n));
  const Usable dist{D, n};
  std::vector<double> a(n, 0.0), s(n, 0.0), b(n, 0.0);
  for (size_t i = 0; i < n; ++i)
    if (valid[i]) a[i] = 1.0 / static_cast<double>(nv);
  for (size_t it = 0; it < iters; ++it) {
    const double q = dist_quadratic(dist, valid, a, s);
    double tot = 0.0;
    for (size_t i = 0; i < n; ++i) {
      if (!valid[i]) continue;
      b[i] = 1.0 / std::max(std::sqrt(std::max(s[i] - q, 0.0)), nu);
      tot += b[i];
    }
    for (size_t i = 0; i < n; ++i)
      if (valid[i]) a[i] = b[i] / tot;
  }
  std::vector<float> w(n, 0.f);
  for (size_t i = 0; i < n; ++i) w[i] = static_cast<float>(a[i]);
  return w;
}

// DnC spectral filtering on the distance matrix alone (docs/GAR_SEMANTICS.md "Spectral filtering"):
// exactly `iters` power rounds on K = -½ J D J (never stored), every sum in index order over the
// valid rows; the min(m, |V|) lowest fp32 scores are kept.
std::vector<float> dnc_weights(const std::vector<double>& D, size_t n, size_t m, size_t iters,
                               std::vector<float>* scores_out) {
  const auto [valid, nv] = valid_rows(D, n, n);
  if (nv == 0) {
    if (scores_out) scores_out->assign(n, 0.f);
    return std::vector<float>(n, static_cast<float>(1.0 / static_cast<double>(n)));
  }
  const Usable dist{D, n};
  const double nvd = static_cast<double>(nv);
  const size_t kv = std::min(m, nv);
  std::vector<double> r(n, 0.0), b(n, 0.0), u(n, 0.0), t(n, 0.0);
  for (size_t i = 0; i < n; ++i) {
    if (!valid[i]) continue;
    double acc = 0.0;
    for (size_t j = 0; j < n; ++j)
      if (valid[j]) acc += dist(i, j);
    r[i] = acc / nvd;
  }
  double g = 0.0;
  for (size_t i = 0; i < n; ++i)
    if (valid[i]) g += r[i];
  g /= nvd;
  size_t star = n;   // the lowest valid index that attains max κ, κ_i = r_i - g/2
  for (size_t i = 0; i < n; ++i)
    if (valid[i] && (star == n || r[i] - 0.5 * g > r[star] - 0.5 * g)) star = i;
  for (size_t i = 0; i < n; ++i)
    if (valid[i]) b[i] = -0.5 * (dist(i, star) - r[i] - r[star] + g);
  for (size_t it = 0; it < iters; ++it) {
    double nu = 0.0;
    for (size_t i = 0; i < n; ++i)
      if (valid[i]) nu += b[i] * b[i];
    nu = std::sqrt(nu);
    double c = 0.0;
    for (size_t i = 0; i < n; ++i) {
      if (!valid[i]) continue;
      u[i] = nu > 0.0 ? b[i] / nu : 0.0;
      c += u[i];
    }
    c /= nvd;
    double tm = 0.0;
    for (size_t i = 0; i < n; ++i) {
      if (!valid[i]) continue;
      double acc = 0.0;
      for (size_t j = 0; j < n; ++j)
        if (valid[j]) acc += dist(i, j) * (u[j] - c);
      t[i] = acc;
      tm += acc;
    }
    tm /= nvd;
    for (size_t i = 0; i < n; ++i)
      if (valid[i]) b[i] = -0.5 * (t[i] - tm);
  }
  double lam = 0.0;
  for (size_t i = 0; i < n; ++i)
    if (valid[i]) lam += u[i] * b[i];
  std::vector<float> s(n, static_cast<float>(kInf));
  for (size_t i = 0; i < n; ++i)
    if (valid[i]) s[i] = lam > 0.0 ? static_cast<float>(b[i] * b[i] / lam) : 0.f;
  std::vector<size_t> order;
  for (size_t i = 0; i < n; ++i)
    if (valid[i]) order.push_back(i);
  std::sort(order.begin(), order.end(), [&](size_t a, size_t c) { return key_less(s[a], a, s[c], c); });
  std::vector<float> w(n, 0.f);
  for (size_t k = 0; k < kv; ++k) w[order[k]] = static_cast<float>(1.0 / static_cast<double>(kv));
  if (scores_out) *scores_out = s;
  return w;
}

// CAF covariance filter on the distance matrix alone (docs/GAR_SEMANTICS.md "Covariance filter"): per
// pass `iters` power rounds on M = A^½ K A^½, K_ij = (x_i - μ_a)·(x_j - μ_a) (never stored), every sum in
// index order over the valid rows; the weights of the pass of smallest λ are kept.
std::vector<float> caf_weights(const std::vector<double>& D, size_t n, size_t f, size_t iters, size_t max_passes,
                               std::vector<float>* lams_out) {
  const auto [valid, nv] = valid_rows(D, n, n);
  std::vector<float> lams(n, static_cast<float>(kInf));
  if (nv == 0) {
    if (lams_out) *lams_out = lams;
    return std::vector<float>(n, static_cast<float>(1.0 / static_cast<double>(n)));
  }
  const Usable dist{D, n};
  if (max_passes == 0 || max_passes > n) max_passes = n;
  const double keep_above = static_cast<double>(n) - 2.0 * static_cast<double>(f);
  std::vector<double> c(n, 0.0), a(n, 0.0), ra(n, 0.0), s(n, 0.0), p(n, 0.0), b(n, 0.0), u(n, 0.0), kp(n, 0.0),
      best_a(n, 0.0);
  for (size_t i = 0; i < n; ++i) c[i] = valid[i] ? 1.0 : 0.0;
  double q = 0.0;
  // kp = K p = -½ (D p - s Σp - (s·p) 1 + q Σp 1) on the valid rows
  auto apply_K = [&]() {
    double sp = 0.0, sdp = 0.0;
    for (size_t i = 0; i < n; ++i)
      if (valid[i]) { sp += p[i]; sdp += s[i] * p[i]; }
    for (size_t i = 0; i < n; ++i) {
      if (!valid[i]) continue;
      double acc = 0.0;
      for (size_t j = 0; j < n; ++j)
        if (valid[j]) acc += dist(i, j) * p[j];
      kp[i] = -0.5 * (acc - s[i] * sp - sdp + q * sp);
    }
  };
  double best = kInf;
  for (size_t pass = 0;; ++pass) {
    double sc = 0.0;
    for (size_t i = 0; i < n; ++i) sc += c[i];
    if (pass == 0)
      for (size_t i = 0; i < n; ++i) best_a[i] = c[i] / sc;
    if (!(sc > keep_above && pass < max_passes)) break;
    for (size_t i = 0; i < n; ++i) {
      a[i] = c[i] / sc;
      ra[i] = std::sqrt(a[i]);
    }
    q = 2.0 * dist_quadratic(dist, valid, a, s);
    size_t star = 0;   // the lowest index that attains max a_i (s_i - q/2)
    for (size_t i = 1; i < n; ++i)
      if (a[i] * (s[i] - 0.5 * q) > a[star] * (s[star] - 0.5 * q)) star = i;
    std::fill(p.begin(), p.end(), 0.0);
    p[star] = ra[star];
    apply_K();
    for (size_t i = 0; i < n; ++i) b[i] = ra[i] * kp[i];
    for (size_t it = 0; it < iters; ++it) {
      double nb = 0.0;
      for (size_t i = 0; i < n; ++i) nb += b[i] * b[i];
      nb = std::sqrt(nb);
      for (size_t i = 0; i < n; ++i) {
        u[i] = nb > 0.0 ? b[i] / nb : 0.0;
        p[i] = ra[i] * u[i];
      }
      apply_K();
      for (size_t i = 0; i < n; ++i) b[i] = ra[i] * kp[i];
    }
    double lam = 0.0;
    for (size_t i = 0; i < n; ++i) lam += u[i] * b[i];
    if (lam < best) {   // strict: the first pass wins a tie
      best = lam;
      best_a = a;
    }
    lams[pass] = static_cast<float>(lam);
    double tmax = 0.0;   // over the rows that still carry weight
    for (size_t i = 0; i < n; ++i)
      if (c[i] > 0.0 && lam > 0.0) tmax = std::max(tmax, kp[i] * kp[i] / lam);
    if (!(lam > 0.0 && tmax > 0.0)) break;
    for (size_t i = 0; i < n; ++i)
      if (c[i] > 0.0) c[i] *= 1.0 - std::min(kp[i] * kp[i] / lam / tmax, 1.0);
  }
  std::vector<float> w(n, 0.f);
  for (size_t i = 0; i < n; ++i) w[i] = static_cast<float>(best_a[i]);
  if (lams_out) *lams_out = lams;
  return w;
}

// Centered clipping on the distance matrix alone (docs/GAR_SEMANTICS.md "Centered clipping"):
// exactly `iters` rounds, every sum in index order.
std::vector<float> cclip_weights(const std::vector<double>& D, size_t n, size_t nw, const std::vector<double>& a0,
                                 double tau, size_t f, size_t iters) {
  const auto [valid, nv] = valid_rows(D, n, nw);   // |V|: the valid workers
  std::vector<float> w(n, 0.f);
  if (nv == 0) {
    for (size_t i = 0; i < nw; ++i) w[i] = static_cast<float>(1.0 / static_cast<double>(nw));
    return w;
  }
  const Usable dist{D, n};
  const double nvd = static_cast<double>(nv);
  std::vector<double> a(n, 0.0), s(n, 0.0), r(n, 0.0), lam(n, 0.0);
  double tot = 0.0;
  if (!a0.empty())
    for (size_t i = 0; i < n; ++i)
      if (valid[i]) tot += (a[i] = a0[i]);
  if (!a0.empty() && std::isfinite(tot) && tot > 0.0) {
    for (size_t i = 0; i < n; ++i) a[i] /= tot;
  } else {
    for (size_t i = 0; i < n; ++i) a[i] = (i < nw && valid[i]) ? 1.0 / nvd : 0.0;
  }
  const size_t k = nv > f ? nv - f : 1;
  for (size_t it = 0; it < iters; ++it) {
    const double q = dist_quadratic(dist, valid, a, s);
    for (size_t i = 0; i < nw; ++i)
      if (valid[i]) r[i] = std::sqrt(std::max(s[i] - q, 0.0));
    double t = tau;
    if (!(tau > 0.0)) {   // the k-th smallest r over V: only its value is used
      std::vector<double> rs;
      for (size_t i = 0; i < nw; ++i)
        if (valid[i]) rs.push_back(r[i]);
      std::nth_element(rs.begin(), rs.begin() + (k - 1), rs.end());
      t = rs[k - 1];
    }
    double Lam = 0.0;
    for (size_t i = 0; i < nw; ++i) {
      if (!valid[i]) continue;
      lam[i] = r[i] <= t ? 1.0 : t / r[i];
      Lam += lam[i];
    }
    const double keep = 1.0 - Lam / nvd;
    for (size_t i = 0; i < n; ++i) a[i] = a[i] * keep + lam[i] / nvd;
  }
  for (size_t i = 0; i < n; ++i) w[i] = static_cast<float>(a[i]);
  return w;
}

// Nearest-neighbour mixing (docs/GAR_SEMANTICS.md "Nearest-neighbour mixing"): the oracle's sums in
// the oracle's order (set members ascending, the inner sum over l first).
std::vector<uint64_t> nnm_sets(const std::vector<double>& D, size_t n, size_t f) {
  const size_t c = n - f;
  const double inf = std::numeric_limits<double>::infinity();
  auto d0 = [&](size_t k, size_t l) {
    const double v = D[k * n + l];
    return k == l ? 0.0 : (std::isfinite(v) ? v : inf);
  };
  std::vector<uint64_t> mk(2 * n, 0);
  for (size_t i = 0; i < n; ++i) {
    mk[2 * i + (i >> 6)] |= uint64_t{1} << (i & 63);
    for (size_t j = 0; j < n; ++j) {
      if (j == i) continue;
      const double dj = d0(i, j);
      size_t rank = 0;
      for (size_t k = 0; k < n; ++k) {
        if (k == i) continue;
        const double dk = d0(i, k);
        rank += dk < dj || (dk == dj && k < j);
      }
      if (rank + 1 < c) mk[2 * i + (j >> 6)] |= uint64_t{1} << (j & 63);
    }
  }
  return mk;
}

std::vector<double> nnm_mix(const std::vector<double>& D, size_t n, size_t f, std::vector<uint64_t>* masks) {
  const size_t c = n - f;
  const double inf = std::numeric_limits<double>::infinity();
  auto d0 = [&](size_t k, size_t l) {
    const double v = D[k * n + l];
    return k == l ? 0.0 : (std::isfinite(v) ? v : inf);
  };
  std::vector<uint64_t> mk = nnm_sets(D, n, f);
  auto has = [&](size_t i, size_t j) { return (mk[2 * i + (j >> 6)] >> (j & 63)) & 1u; };
  std::vector<double> R(n * n, 0.0);   // R[j * n + k] = Σ_{l∈S_j} D⁰_kl
  for (size_t j = 0; j < n; ++j)
    for (size_t k = 0; k < n; ++k) {
      double acc = 0.0;
      for (size_t l = 0; l < n; ++l)
        if (has(j, l)) acc += d0(k, l);
      R[j * n + k] = acc;
    }
  auto m_of = [&](size_t i, size_t j) {
    double acc = 0.0;
    for (size_t k = 0; k < n; ++k)
      if (has(i, k)) acc += R[j * n + k];
    return acc / (static_cast<double>(c) * static_cast<double>(c));
  };
  std::vector<double> diag(n);
  for (size_t i = 0; i < n; ++i) diag[i] = m_of(i, i);
  std::vector<double> out(n * n, inf);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = i + 1; j < n; ++j) {
      const double mij = m_of(i, j);
      double v = inf;
      if (!std::isinf(mij) && !std::isinf(diag[i]) && !std::isinf(diag[j]))
        v = std::max(mij - 0.5 * diag[i] - 0.5 * diag[j], 0.0);
      out[i * n + j] = out[j * n + i] = v;
    }
  if (masks) *masks = std::move(mk);
  return out;
}

std::vector<float> nnm_unmix(const std::vector<float>& a, const std::vector<uint64_t>& masks, size_t n, size_t c) {
  std::vector<double> acc(n, 0.0);
  double tot = 0.0;   // the fp32 a sum to 1 only within rounding: w is normalised by their fp64 sum
  for (size_t i = 0; i < n; ++i) {
    if (a[i] == 0.f) continue;
    tot += static_cast<double>(a[i]);
    for (size_t j = 0; j < n; ++j)
      if ((masks[2 * i + (j >> 6)] >> (j & 63)) & 1u) acc[j] += static_cast<double>(a[i]);
  }
  std::vector<float> w(n, 0.f);
  if (tot == 0.0) return w;
  for (size_t j = 0; j < n; ++j) w[j] = static_cast<float>(acc[j] / tot / static_cast<double>(c));
  return w;
}

std::vector<float> bulyan_weights(const std::vector<double>& D, size_t n, size_t f, size_t m, size_t t) {
  const size_t q = n - f - 2;
  std::vector<double> scores(n, 0.0);
  std::vector<double> P(n * n, 0.0);  // pruned distances: only each row's q nearest survive
  for (size_t i = 0; i < n; ++i) {
    double s = 0.0;
    for (size_t j : nearest(D, n, i, q)) {
      s += D[i * n + j];
      P[i * n + j] = D[i * n + j];
    }
    scores[i] = s;
  }
  std::vector<float> W(t * n, 0.f);
  for (size_t k = 0; k < t; ++k) {
    const size_t mk = (m > k) ? m - k : 1;
    const auto order = rank_order(scores);
    for (size_t r = 0; r < mk && r < n; ++r) W[k * n + order[r]] = 1.f / static_cast<float>(mk);
    const size_t id = order[0];
    for (size_t i = 0; i < n; ++i)
      if (i != id) scores[i] -= P[i * n + id];
    scores[id] = static_cast<double>(FLT_MAX);
  }
  return W;
}

static unsigned long long binom(size_t a, size_t b) {
  if (b > a) return 0ull;
  if (b > a - b) b = a - b;
  unsigned long long r = 1;
  for (size_t i = 1; i <= b; ++i) r = r * static_cast<unsigned long long>(a - b + i) / i;
  return r;
}

static unsigned long long unrank_mask(unsigned long long r, size_t n, size_t k) {
  unsigned long long mask = 0ull;
  for (size_t ii = n; ii-- > 0 && k > 0;) {
    const unsigned long long c = binom(ii, k);
    if (c <= r) {
      mask |= 1ull << ii;
      r -= c;
      --k;
    }
  }
  return mask;
}

std::vector<float> brute_weights(const std::vector<double>& D, size_t n, size_t f) {
  if (n > 64) throw std::invalid_argument("brute: n must be <= 64");
  const size_t k = n - f;
  const unsigned long long total = binom(n, k);
  // distances as fp32 (non-finite -> FLT_MAX), exactly as the device search
  std::vector<float> Df(n * n);
  for (size_t e = 0; e < n * n; ++e) {
    const double v = D[e];
    Df[e] = std::isfinite(v) ? static_cast<float>(std::max(v, 0.0)) : FLT_MAX;
  }
  const size_t nchunks = static_cast<size_t>(std::min<unsigned long long>(total, 256ull));
  std::vector<std::pair<float, unsigned long long>> best(nchunks, {FLT_MAX, ~0ull});
  parallel_for(0, static_cast<size_t>(total), nchunks, [&](size_t c, size_t lo, size_t hi) {
    unsigned long long mask = unrank_mask(lo, n, k);
    std::pair<float, unsigned long long> b{std::numeric_limits<float>::infinity(), ~0ull};
    for (size_t rank = lo; rank < hi; ++rank) {
      float diam = 0.f;
      for (unsigned long long mi = mask; mi;) {
        const int i = __builtin_ctzll(mi);
        mi &= mi - 1ull;
        for (unsigned long long mj = mi; mj;) {
          const int j = __builtin_ctzll(mj);
          mj &= mj - 1ull;
          diam = std::max(diam, Df[static_cast<size_t>(i) * n + static_cast<size_t>(j)]);
        }
      }
      if (diam < b.first || (diam == b.first && rank < b.second)) b = {diam, rank};
      const unsigned long long cc = mask & (~mask + 1ull);
      const unsigned long long rr = mask + cc;
      mask = (((rr ^ mask) >> 2) / cc) | rr;
    }
    best[c] = b;
  });
  auto b = best[0];
  for (auto& x : best)
    if (x.first < b.first || (x.first == b.first && x.second < b.second)) b = x;
  const unsigned long long mask = unrank_mask(b.second, n, k);
  std::vector<float> w(n, 0.f);
  for (size_t i = 0; i < n; ++i)
    if ((mask >> i) & 1ull) w[i] = 1.f / static_cast<float>(k);
  return w;
}

// SMEA (docs/GAR_SEMANTICS.md "SMEA"): Brute's enumeration, every subset scored by exactly `iters` power
// rounds on K_S = -½ J D_S J of its k x k block of the distances (the loop of dnc_weights on the members in
// increasing index, every sum in index order), λ / k as fp32; the smallest (λ bits, rank) key wins.
std::vector<float> smea_weights(const std::vector<double>& D, size_t n, size_t f, size_t iters, float* lam_out) {
  if (n > 64) throw std::invalid_argument("smea: n must be <= 64");
  const size_t k = n - f;
  const unsigned long long total = binom(n, k);
  if (total >> 32) throw std::invalid_argument("smea: more than 2^32 subsets");
  // clamped at 0, a zero diagonal, +inf where non-finite (a subset with such a pair scores +inf)
  std::vector<double> Dc(n * n);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) {
      const double v = D[i * n + j];
      Dc[i * n + j] = i == j ? 0.0 : (std::isfinite(v) ? std::max(v, 0.0) : kInf);
    }
  const double kd = static_cast<double>(k);
  const size_t nchunks = static_cast<size_t>(std::min<unsigned long long>(total, 256ull));
  std::vector<unsigned long long> best(nchunks, ~0ull);
  parallel_for(0, static_cast<size_t>(total), nchunks, [&](size_t c, size_t lo, size_t hi) {
    unsigned long long mask = unrank_mask(lo, n, k);
    unsigned long long mine = ~0ull;
    std::vector<size_t> S(k);
    std::vector<double> B(k * k), r(k), b(k), u(k), t(k);
    for (size_t rank = lo; rank < hi; ++rank) {
      size_t q = 0;
      for (unsigned long long mi = mask; mi; mi &= mi - 1ull) S[q++] = static_cast<size_t>(__builtin_ctzll(mi));
      bool finite = true;
      for (size_t p = 0; p < k; ++p)
        for (size_t j = 0; j < k; ++j) {
          B[p * k + j] = Dc[S[p] * n + S[j]];
          finite = finite && std::isfinite(B[p * k + j]);
        }
      float score = static_cast<float>(kInf);
      if (finite) {
        for (size_t p = 0; p < k; ++p) {
          double acc = 0.0;
          for (size_t j = 0; j < k; ++j) acc += B[p * k + j];
          r[p] = acc / kd;
        }
        double g = 0.0;
        for (size_t p = 0; p < k; ++p) g += r[p];
        g /= kd;
        size_t star = 0;   // the lowest position that attains max κ, κ_p = r_p - g/2
        for (size_t p = 1; p < k; ++p)
          if (r[p] - 0.5 * g > r[star] - 0.5 * g) star = p;
        for (size_t p = 0; p < k; ++p) b[p] = -0.5 * (B[p * k + star] - r[p] - r[star] + g);
        std::fill(u.begin(), u.end(), 0.0);
        for (size_t it = 0; it < iters; ++it) {
          double nu = 0.0;
          for (size_t p = 0; p < k; ++p) nu += b[p] * b[p];
          nu = std::sqrt(nu);
          double cm = 0.0;
          for (size_t p = 0; p < k; ++p) {
            u[p] = nu > 0.0 ? b[p] / nu : 0.0;
            cm += u[p];
          }
          cm /= kd;
          double tm = 0.0;
          for (size_t p = 0; p < k; ++p) {
            double acc = 0.0;
            for (size_t j = 0; j < k; ++j) acc += B[p * k + j] * (u[j] - cm);
            t[p] = acc;
            tm += acc;
          }
          tm /= kd;
          for (size_t p = 0; p < k; ++p) b[p] = -0.5 * (t[p] - tm);
        }
        double lam = 0.0;
        for (size_t p = 0; p < k; ++p) lam += u[p] * b[p];
        score = static_cast<float>(lam / kd);
        if (!(score >= 0.f)) score = score < 0.f ? 0.f : static_cast<float>(kInf);   // negative: 0; NaN: +inf
      }
      uint32_t bits;
      std::memcpy(&bits, &score, sizeof bits);
      const unsigned long long key = (static_cast<unsigned long long>(bits) << 32) | rank;
      if (key < mine) mine = key;
      const unsigned long long cc = mask & (~mask + 1ull);
      const unsigned long long rr = mask + cc;
      mask = (((rr ^ mask) >> 2) / cc) | rr;
    }
    best[c] = mine;
  });
  unsigned long long key = best[0];   // reduced in a fixed order
  for (size_t c = 1; c < nchunks; ++c) key = std::min(key, best[c]);
  const unsigned long long mask = unrank_mask(key & 0xffffffffull, n, k);
  std::vector<float> w(n, 0.f);
  for (size_t i = 0; i < n; ++i)
    if ((mask >> i) & 1ull) w[i] = 1.f / static_cast<float>(k);
  if (lam_out) {
    const uint32_t bits = static_cast<uint32_t>(key >> 32);
    std::memcpy(lam_out, &bits, sizeof bits);
  }
  return w;
}

std::vector<float> aksel_weights(const std::vector<double>& dists, size_t n, size_t c) {
  const auto order = rank_order(dists);
  std::vector<float> w(n, 0.f);
  for (size_t r = 0; r < c && r < n; ++r) w[order[r]] = 1.f / static_cast<float>(c);
  return w;
}

template <class T>
void combine(const Rows<T>& r, const std::vector<float>& w, T* out) {
  std::vector<size_t> sel;
  for (size_t j = 0; j < r.n; ++j)
    if (w[j] != 0.f) sel.push_back(j);
  parallel_for(0, r.d, default_chunks(r.d), [&](size_t, size_t lo, size_t hi) {
    for (size_t x = lo; x < hi; ++x) {
      double s = 0.0;
      for (size_t j : sel) s += static_cast<double>(w[j]) * static_cast<double>(r.p[j][x]);
      out[x] = static_cast<T>(s);
    }
  });
}

// Mean of the beta values of v closest to the median v[len/2] of the sorted v;
// ties broken by value (the GPU network's (key, value) order).
static double closest_mean(std::vector<double>& v, size_t len, size_t beta) {
  std::sort(v.begin(), v.begin() + static_cast<long>(len));
  const double med = v[len / 2];
  std::vector<std::pair<double, double>> kv(len);
  for (size_t i = 0; i < len; ++i) kv[i] = {nan_to_inf(std::fabs(v[i] - med)), v[i]};
  std::sort(kv.begin(), kv.end());
  double s = 0.0;
  for (size_t i = 0; i < beta && i < len; ++i) s += kv[i].second;
  return s / static_cast<double>(beta);
}

template <class T>
void coordwise(const Rows<T>& r, int mode, size_t f, size_t beta, const std::vector<float>& W, size_t t,
               uint64_t seed, uint64_t threshold, T* out) {
  const size_t n = r.n;
  parallel_for(0, r.d, default_chunks(r.d, 1024), [&](size_t, size_t lo, size_t hi) {
    std::vector<double> v(std::max(n, t) + 1);
    for (size_t x = lo; x < hi; ++x) {
      double res = 0.0;
      switch (mode) {
        case kAverageNan: {
          double s = 0.0;
          size_t c = 0;
          for (size_t i = 0; i < n; ++i) {
            const double a = static_cast<double>(r.p[i][x]);
            if (std::isfinite(a)) { s += a; ++c; }
          }
          res = c ? s / static_cast<double>(c) : 0.0;
          break;
        }
        case kMedian:
        case kCondense: {
          size_t c = 0;
          for (size_t i = 0; i < n; ++i) {
            const double a = static_cast<double>(r.p[i][x]);
            if (std::isfinite(a)) v[c++] = a;
          }
          if (c) {
            std::nth_element(v.begin(), v.begin() + static_cast<long>(c / 2), v.begin() + static_cast<long>(c));
            res = v[c / 2];
          }
          if (mode == kCondense) {
            const uint32_t draw = mix_hash(seed, static_cast<uint64_t>(x));
            if (!(static_cast<uint64_t>(draw) < threshold)) res = static_cast<double>(r.p[0][x]);
          }
          break;
        }
        case kTrimmedMean: {
          for (size_t i = 0; i < n; ++i) v[i] = nan_to_inf(static_cast<double>(r.p[i][x]));
          std::sort(v.begin(), v.begin() + static_cast<long>(n));
          double s = 0.0;
          for (size_t i = f; i < n - f; ++i) s += v[i];
          res = s / static_cast<double>(n - 2 * f);
          break;
        }
        case kAveragedMedian: {
          for (size_t i = 0; i < n; ++i) v[i] = nan_to_inf(static_cast<double>(r.p[i][x]));
          res = closest_mean(v, n, beta);
          break;
        }
        case kBulyanTail: {
          for (size_t k = 0; k < t; ++k) {
            double s = 0.0;
            for (size_t j = 0; j < n; ++j) {
              const float w = W[k * n + j];
              if (w != 0.f) s += static_cast<double>(w) * static_cast<double>(r.p[j][x]);
            }
            v[k] = nan_to_inf(s);
          }
          res = closest_mean(v, t, beta);
          break;
        }
        default:
          throw std::invalid_argument("coordwise: unknown mode");
      }
      out[x] = static_cast<T>(res);
    }
  });
}

// NNM before a coordinate-wise rule: per coordinate, the n set means (fp64 sums over the members in
// ascending index, then / c) and coordwise()'s trimmed mean / median over them. Nothing depends on
// where a coordinate sits in a chunk: any column split of the rows gives the same bits.
template <class T>
void mixed_coordwise(const Rows<T>& r, const std::vector<uint64_t>& masks, size_t c, int mode, size_t f, T* out) {
  const size_t n = r.n;
  if (mode != kTrimmedMean && mode != kMedian) throw std::invalid_argument("mixed_coordwise: trimmed mean or median");
  std::vector<std::vector<size_t>> sets(n);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j)
      if ((masks[2 * i + (j >> 6)] >> (j & 63)) & 1u) sets[i].push_back(j);
  const double cd = static_cast<double>(c);
  parallel_for(0, r.d, default_chunks(r.d, 1024), [&](size_t, size_t lo, size_t hi) {
    std::vector<double> g(n), v(n);
    for (size_t x = lo; x < hi; ++x) {
      for (size_t j = 0; j < n; ++j) g[j] = static_cast<double>(r.p[j][x]);
      double res = 0.0;
      if (mode == kMedian) {
        size_t cnt = 0;
        for (size_t i = 0; i < n; ++i) {
          double s = 0.0;
          for (size_t j : sets[i]) s += g[j];
          s /= cd;
          if (std::isfinite(s)) v[cnt++] = s;
        }
        if (cnt) {
          std::nth_element(v.begin(), v.begin() + static_cast<long>(cnt / 2), v.begin() + static_cast<long>(cnt));
          res = v[cnt / 2];
        }
      } else {
        for (size_t i = 0; i < n; ++i) {
          double s = 0.0;
          for (size_t j : sets[i]) s += g[j];
          v[i] = nan_to_inf(s / cd);
        }
        std::sort(v.begin(), v.end());
        double s = 0.0;
        for (size_t i = f; i < n - f; ++i) s += v[i];
        res = s / static_cast<double>(n - 2 * f);
      }
      out[x] = static_cast<T>(res);
    }
  });
}

template <class T>
std::vector<double> sqdist_to(const Rows<T>& r, const T* center) {
  const size_t n = r.n;
  const size_t nchunks = default_chunks(r.d);
  std::vector<double> partial(nchunks * n, 0.0);
  parallel_for(0, r.d, nchunks, [&](size_t c, size_t lo, size_t hi) {
    for (size_t j = 0; j < n; ++j) {
      double s = 0.0;
      for (size_t x = lo; x < hi; ++x) {
        const double a = static_cast<double>(r.p[j][x]) - static_cast<double>(center[x]);
        s += a * a;
      }
      partial[c * n + j] = s;
    }
  });
  std::vector<double> out(n, 0.0);
  for (size_t j = 0; j < n; ++j) {
    double s = 0.0;
    for (size_t c = 0; c < nchunks; ++c) s += partial[c * n + j];
    out[j] = std::isfinite(s) ? s : kInf;
  }
  return out;
}

// ---------------------------------------------------------------------------
// Worker-side momentum (docs/GAR_SEMANTICS.md "Worker momentum"; the kernel: worker_mom.hip)

namespace {

inline uint32_t f32_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline float bits_f32(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

inline float bf16_widen(uint16_t h) { return bits_f32(static_cast<uint32_t>(h) << 16); }
// round-to-nearest-even of a finite value (a carry out of the mantissa gives the next exponent, up to inf)
inline uint16_t bf16_round(float f) {
  const uint32_t u = f32_bits(f);
  return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

inline float f16_widen(uint16_t h) {
  const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  if (e == 0) return bits_f32(f32_bits(static_cast<float>(m) * 0x1p-24f) | sign);   // zero and subnormals
  if (e == 31) return bits_f32(sign | 0x7f800000u | (m << 13));
  return bits_f32(sign | ((e + 112u) << 23) | (m << 13));
}
// round-to-nearest-even of a finite value; 65520 and above give inf
inline uint16_t f16_round(float f) {
  uint32_t u = f32_bits(f);
  const uint16_t sign = static_cast<uint16_t>((u >> 16) & 0x8000u);
  u &= 0x7fffffffu;
  if (u >= 0x47800000u) return sign | 0x7c00u;
  if (u < 0x38800000u)   // below 2^-14: the sum with 0.5 rounds the subnormal mantissa in place
    return sign | static_cast<uint16_t>(f32_bits(bits_f32(u) + 0.5f) - 0x3f000000u);
  const uint32_t odd = (u >> 13) & 1u;
  u += 0xc8000fffu + odd;   // exponent bias 127 -> 15, and the rounding bias
  return sign | static_cast<uint16_t>(u >> 13);
}

template <int DT> struct RowElem;
template <> struct RowElem<kF32> {
  using type = float;
  static float widen(float v) { return v; }
  static float round(float m) { return m; }
};
template <> struct RowElem<kBF16> {
  using type = uint16_t;
  static float widen(uint16_t v) { return bf16_widen(v); }
  static uint16_t round(float m) { return bf16_round(m); }
};
template <> struct RowElem<kF16> {
  using type = uint16_t;
  static float widen(uint16_t v) { return f16_widen(v); }
  static uint16_t round(float m) { return f16_round(m); }
};

template <int DT>
void worker_momentum_t(void* X, int64_t xstride, float* M, int64_t ld, size_t k, size_t lo, size_t hi, float beta,
                       float omega, bool first) {
  using E = typename RowElem<DT>::type;
  parallel_for(lo, hi, default_chunks(hi - lo), [&](size_t, size_t a, size_t b) {
    for (size_t r = 0; r < k; ++r) {
      E* row = static_cast<E*>(X) + static_cast<int64_t>(r) * xstride;
      float* m = M + static_cast<int64_t>(r) * ld;
      for (size_t x = a; x < b; ++x) {
        const float g = RowElem<DT>::widen(row[x]);
        if (!std::isfinite(g)) continue;   // the row keeps it, the state stays
        const float prod = omega * g;
        m[x] = first ? g : std::fmaf(beta, m[x], prod);
        row[x] = RowElem<DT>::round(m[x]);
      }
    }
  });
}

}  // namespace

void worker_momentum(void* X, int dt, int64_t xstride, float* M, int64_t ld, size_t k, size_t lo, size_t hi, float beta,
                     float omega, bool first) {
  if (k == 0 || hi <= lo) return;
  if (dt == kF32) worker_momentum_t<kF32>(X, xstride, M, ld, k, lo, hi, beta, omega, first);
  else if (dt == kBF16) worker_momentum_t<kBF16>(X, xstride, M, ld, k, lo, hi, beta, omega, first);
  else if (dt == kF16) worker_momentum_t<kF16>(X, xstride, M, ld, k, lo, hi, beta, omega, first);
  else throw std::invalid_argument("worker_momentum: fp32, bf16 or fp16 rows");
}

#define GARFIELD_INSTANTIATE(T)                                                                          \
  template std::vector<double> pairwise_sqdist<T>(const Rows<T>&);                                       \
  template void combine<T>(const Rows<T>&, const std::vector<float>&, T*);                               \
  template void coordwise<T>(const Rows<T>&, int, size_t, size_t, const std::vector<float>&, size_t,     \
                             uint64_t, uint64_t, T*);                                                    \
  template void mixed_coordwise<T>(const Rows<T>&, const std::vector<uint64_t>&, size_t, int, size_t, T*); \
  template std::vector<double> sqdist_to<T>(const Rows<T>&, const T*);

GARFIELD_INSTANTIATE(float)
GARFIELD_INSTANTIATE(double)
#undef GARFIELD_INSTANTIATE

}  // namespace cpu
}  // namespace garfield

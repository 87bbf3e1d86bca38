// Host-side self-test of the native CPU runtime, built with -fsanitize=thread or
// -fsanitize=address by tests/test_native_sanitizers.py (race / memory-error
// detection: the reference had none). Exercises:
//  * ThreadPool::run_chunks from several caller threads at once (the completion
//    protocol that once let a waiter destroy its condvar under a notifier);
//  * the CPU GARs (pairwise distances, Krum / Bulyan / Brute selections,
//    coordinate-wise rules) against simple serial recomputations;
//  * Mailbox: concurrent writers publishing tagged slots while a reader waits.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <thread>
#include <vector>

#include "gar_common.hpp"
#include "gar_cpu.hpp"
#include "mailbox.hpp"
#include "threadpool.hpp"

using namespace garfield;

static int failures = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static void test_pool() {
  std::vector<std::thread> callers;
  std::atomic<long> total{0};
  for (int c = 0; c < 6; ++c) {
    callers.emplace_back([&total] {
      for (int rep = 0; rep < 200; ++rep) {
        std::vector<long> part(37, 0);
        cpu::parallel_for(0, 10000, 37, [&](size_t chunk, size_t lo, size_t hi) {
          long s = 0;
          for (size_t i = lo; i < hi; ++i) s += static_cast<long>(i);
          part[chunk] = s;
        });
        long s = 0;
        for (long p : part) s += p;
        total += s;
      }
    });
  }
  for (auto& t : callers) t.join();
  CHECK(total.load() == 6L * 200L * (9999L * 10000L / 2));
}

static void test_gars() {
  std::mt19937 rng(7);
  std::normal_distribution<float> nd;
  const size_t n = 11, d = 3001, f = 2;
  std::vector<std::vector<float>> data(n, std::vector<float>(d));
  for (size_t i = 0; i < n; ++i)
    for (size_t x = 0; x < d; ++x) data[i][x] = nd(rng) * (1.0f + 0.3f * static_cast<float>(i));
  cpu::Rows<float> r;
  r.n = n;
  r.d = d;
  for (auto& v : data) r.p.push_back(v.data());
  auto D = cpu::pairwise_sqdist(r);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) {
      if (i == j) continue;
      double s = 0;
      for (size_t x = 0; x < d; ++x) {
        const double a = static_cast<double>(data[i][x]) - data[j][x];
        s += a * a;
      }
      CHECK(std::fabs(D[i * n + j] - s) <= 1e-9 * s);
    }
  auto w = cpu::krum_weights(D, n, f, n - f - 2);
  float tot = 0;
  for (float x : w) tot += x;
  CHECK(std::fabs(tot - 1.f) < 1e-5f);
  auto W = cpu::bulyan_weights(D, n - 2, f, n - 2 - f - 2, n - 2 - 2 * f - 2);
  CHECK(!W.empty());
  auto wb = cpu::brute_weights(D, n, f);
  size_t sel = 0;
  for (float x : wb) sel += x != 0.f;
  CHECK(sel == n - f);
  std::vector<float> out(d);
  cpu::coordwise<float>(r, kMedian, 0, 0, {}, 0, 0, 0, out.data());
  for (size_t x = 0; x < d; x += 97) {
    std::vector<float> col;
    for (size_t i = 0; i < n; ++i) col.push_back(data[i][x]);
    std::sort(col.begin(), col.end());
    CHECK(out[x] == col[n / 2]);
  }
  cpu::coordwise<float>(r, kTrimmedMean, f, 0, {}, 0, 0, 0, out.data());
  cpu::combine<float>(r, w, out.data());
}

// Nearest-neighbour mixing on a distance matrix of points on a line: rows 0..3 get the same set
// (exact zero distances), row 6 is non-finite (tainted: it takes no weight).
static void test_nnm() {
  const size_t n = 7, f = 2, c = n - f;
  const double inf = std::numeric_limits<double>::infinity();
  const double pos[n] = {0.0, 0.1, 1.0, 1.3, 5.0, 5.2, 0.0};
  std::vector<double> D(n * n, inf);
  for (size_t i = 0; i + 1 < n; ++i)
    for (size_t j = 0; j + 1 < n; ++j)
      if (i != j) D[i * n + j] = (pos[i] - pos[j]) * (pos[i] - pos[j]);
  std::vector<uint64_t> mk;
  auto Dm = cpu::nnm_mix(D, n, f, &mk);
  CHECK(mk.size() == 2 * n);
  for (size_t i = 0; i < n; ++i) {
    CHECK((mk[2 * i] >> i) & 1u);
    CHECK(__builtin_popcountll(mk[2 * i]) == static_cast<int>(c) && mk[2 * i + 1] == 0);
  }
  CHECK(mk[0] == 0x1Fu && mk[2] == 0x1Fu);      // rows 0 and 1: {0, 1, 2, 3, 4}
  CHECK(Dm[0 * n + 1] == 0.0 && Dm[1 * n + 0] == 0.0);
  CHECK(mk[2 * 5] == 0x3Eu);                    // row 5: {1, 2, 3, 4, 5}
  // mixed rows on the line: y_0 = 1.48, y_5 = 2.52
  CHECK(std::fabs(Dm[0 * n + 5] - 1.04 * 1.04) < 1e-12);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) CHECK(Dm[i * n + j] == Dm[j * n + i]);
  for (size_t j = 0; j + 1 < n; ++j) CHECK(std::isinf(Dm[6 * n + j]));   // the tainted row
  auto a = cpu::krum_weights(Dm, n, f, n - f - 2);
  CHECK(a[6] == 0.f);
  auto w = cpu::nnm_unmix(a, mk, n, c);
  float tot = 0;
  for (float x : w) tot += x;
  CHECK(std::fabs(tot - 1.f) < 1e-6f);
  CHECK(w[6] == 0.f && w[5] == 0.f && w[0] == 0.2f);
}

// Centered clipping on points on a line: one round with a radius above every distance lands on the
// exact mean of the valid workers from any start (a centre row keeps no weight); a small radius moves
// the centre by exactly that radius; the non-finite row takes no weight.
static void test_cclip() {
  const size_t n = 6, nw = 5;
  const double inf = std::numeric_limits<double>::infinity();
  const double pos[n] = {0.0, 0.1, 0.2, 10.0, 0.0 /* non-finite */, 3.0 /* the centre */};
  std::vector<double> D(n * n, inf);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j)
      if (i != j && i != 4 && j != 4) D[i * n + j] = (pos[i] - pos[j]) * (pos[i] - pos[j]);
  std::vector<double> at_centre(n, 0.0);
  at_centre[n - 1] = 1.0;
  auto w = cpu::cclip_weights(D, n, nw, at_centre, 1e30, 1, 1);
  for (size_t i = 0; i < 4; ++i) CHECK(w[i] == 0.25f);
  CHECK(w[4] == 0.f && w[5] == 0.f);
  // from the centre at 3.0 with radius 0.5: every worker is farther, so the centre moves by
  // (1/4) (3 x -0.5 + 0.5) = -0.25
  w = cpu::cclip_weights(D, n, nw, at_centre, 0.5, 1, 1);
  double v = 0.0, tot = 0.0;
  for (size_t i = 0; i < n; ++i) {
    v += static_cast<double>(w[i]) * pos[i];
    tot += w[i];
  }
  CHECK(std::fabs(tot - 1.0) < 1e-6 && std::fabs(v - 2.75) < 1e-5 && w[4] == 0.f);
  // the data-derived radius with f = 1 from the mean (2.575): the 3rd smallest distance, 2.575
  w = cpu::cclip_weights(D, n, nw, {}, 0.0, 1, 1);
  v = 0.0;
  for (size_t i = 0; i < n; ++i) v += static_cast<double>(w[i]) * pos[i];
  CHECK(std::fabs(v - (2.575 + 0.25 * (-2.575 - 2.475 - 2.375 + 2.575))) < 1e-5);
}

// The covariance filter on points on a line (the covariance is a scalar, τ_i = (x_i - μ)²): the first pass
// zeroes the farther colluder, the second the other one, the third runs on the honest points alone, has the
// smallest λ and is kept; its update leaves less than n - 2f = 5 rows' worth of weight. The non-finite
// row takes no weight.
static void test_caf() {
  const size_t n = 9, f = 2;
  const double inf = std::numeric_limits<double>::infinity();
  const double pos[n] = {0.0, 0.1, 0.2, 0.3, 0.0 /* non-finite */, 0.15, 0.25, 10.0, 10.1};
  std::vector<double> D(n * n, inf);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j)
      if (i != j && i != 4 && j != 4) D[i * n + j] = (pos[i] - pos[j]) * (pos[i] - pos[j]);
  std::vector<float> lams;
  auto w = cpu::caf_weights(D, n, f, 16, 0, &lams);
  CHECK(w.size() == n && lams.size() == n);
  CHECK(std::isfinite(lams[0]) && std::isfinite(lams[1]) && std::isfinite(lams[2]) && std::isinf(lams[3]));
  CHECK(lams[0] > lams[1] && lams[1] > lams[2] && lams[2] > 0.f);
  CHECK(w[4] == 0.f && w[7] == 0.f && w[8] == 0.f);
  double tot = 0.0;
  for (size_t i = 0; i < n; ++i) {
    CHECK(w[i] >= 0.f);
    tot += w[i];
  }
  CHECK(std::fabs(tot - 1.0) < 1e-6);
  // one pass at most: uniform on the valid rows; f = 0: no pass at all
  w = cpu::caf_weights(D, n, f, 16, 1, &lams);
  for (size_t i = 0; i < n; ++i) CHECK(w[i] == (i == 4 ? 0.f : 0.125f));
  CHECK(std::isfinite(lams[0]) && std::isinf(lams[1]));
  w = cpu::caf_weights(D, n, 0, 16, 0, &lams);
  CHECK(w[0] == 0.125f && w[4] == 0.f && std::isinf(lams[0]));
}

// SMEA on points on a line (the covariance is a scalar: λ of a subset is its members' variance): the five
// honest points win, the two colluders and the non-finite row take no weight; with f = 0 every subset holds
// the non-finite row, scores +inf, and rank 0 (all rows) wins; k = 1 scores 0 and rank 0 is row 0.
static void test_smea() {
  const size_t n = 8, f = 3;
  const double inf = std::numeric_limits<double>::infinity();
  const double pos[n] = {0.0, 0.1, 0.2, 0.3, 0.0 /* non-finite */, 0.15, 10.0, 10.0};
  std::vector<double> D(n * n, inf);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j)
      if (i != j && i != 4 && j != 4) D[i * n + j] = (pos[i] - pos[j]) * (pos[i] - pos[j]);
  float lam = -1.f;
  auto w = cpu::smea_weights(D, n, f, 16, &lam);
  CHECK(w.size() == n);
  for (size_t i = 0; i < n; ++i) CHECK(w[i] == ((i == 4 || i >= 6) ? 0.f : 0.2f));
  CHECK(std::fabs(lam - 0.01f) < 1e-6f);
  w = cpu::smea_weights(D, n, 0, 16, &lam);
  for (size_t i = 0; i < n; ++i) CHECK(w[i] == 0.125f);
  CHECK(std::isinf(lam));
  w = cpu::smea_weights(D, n, n - 1, 16, &lam);
  CHECK(w[0] == 1.f && w[1] == 0.f && lam == 0.f);
}

// Worker momentum on exactly sized buffers (an access outside them is the sanitizer's to find): bf16
// rows with a row stride, a range inside the row; powers of two make every value exact.
static void test_worker_momentum() {
  const size_t k = 3, ld = 10007, stride = 2 * ld, lo = 3, hi = ld - 2;
  std::vector<uint16_t> X(k * stride, 0x4000);   // bf16 2.0 everywhere
  std::vector<float> M(k * ld, 4.0f);
  X[1 * stride + 100] = 0x7fc0;                  // NaN: stays in the row, out of the state
  cpu::worker_momentum(X.data(), kBF16, static_cast<int64_t>(stride), M.data(), static_cast<int64_t>(ld), k, lo, hi,
                       0.5f, 0.5f, false);
  for (size_t r = 0; r < k; ++r)
    for (size_t x = 0; x < ld; ++x) {
      const bool in = x >= lo && x < hi, nan = r == 1 && x == 100;
      CHECK(M[r * ld + x] == (in && !nan ? 3.0f : 4.0f));                       // 0.5 * 4 + 0.5 * 2
      CHECK(X[r * stride + x] == (nan ? 0x7fc0 : (in ? 0x4040 : 0x4000)));      // bf16 3.0 inside the range
      CHECK(X[r * stride + ld + x] == 0x4000);                                  // the other half of the stride
    }
  cpu::worker_momentum(X.data(), kBF16, static_cast<int64_t>(stride), M.data(), static_cast<int64_t>(ld), k, 0, 1, 0.5f,
                       0.5f, true);
  CHECK(M[0] == 2.0f && M[1] == 4.0f && X[0] == 0x4000);                        // first step: m <- g
}

static void test_mailbox() {
  mailbox::Mailbox mb(8, 4096, false);
  std::vector<std::thread> writers;
  for (int it = 1; it <= 50; ++it) {
    writers.clear();
    for (int s = 0; s < 8; ++s) {
      writers.emplace_back([&mb, s, it] {
        std::vector<float> buf(1024, static_cast<float>(it * 100 + s));
        mb.write(static_cast<size_t>(s), it, buf.data(), buf.size() * sizeof(float));
      });
    }
    auto ids = mb.wait(it, 6, 5.0);
    CHECK(ids.size() >= 6);
    for (auto& t : writers) t.join();
    auto all = mb.ready(it);
    CHECK(all.size() == 8);
    for (size_t id : all) CHECK(static_cast<const float*>(mb.slot(id))[1023] == static_cast<float>(it * 100 + id));
  }
}

int main() {
  test_pool();
  test_gars();
  test_nnm();
  test_cclip();
  test_caf();
  test_smea();
  test_worker_momentum();
  test_mailbox();
  if (failures) {
    std::fprintf(stderr, "selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("selftest: ok\n");
  return 0;
}

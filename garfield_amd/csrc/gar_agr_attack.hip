// Adaptive colluding attacks Min-Max / Min-Sum (Shejwalkar & Houmansadr, NDSS 2021) on the exchanged rows.
//
// The k rows of the table are the colluders' estimates E: rows 0..P-1 the peers' honest rows, rows
// P..k-1 the T Byzantine rows, which still hold their honest gradient. Every Byzantine row becomes
// m = μ + γ p, μ the mean over E and p the perturbation (-σ, -μ or -sign μ), with the largest γ that keeps
// m inside the distance ball of E. With a_i = ‖μ - e_i‖², b_i = Σ_x p (μ - e_i) and c = Σ_x p²,
// ‖m - e_i‖² = a_i + 2 γ b_i + γ² c, so γ has a closed form: no bisection, no pass over the rows per probe.
//   k_agr_stats   one streaming pass: b_i and c of the coordinates [lo, hi), one fp64 partial per workgroup
//   k_agr_reduce  the workgroups' partials -> one additive [k + 1] vector (the sharded step sums those)
//   k_agr_solve   one workgroup: Σ partials, a_i from the distances of the Gram, the closed form -> γ
//   k_agr_write   one streaming pass: μ, p recomputed per coordinate, every Byzantine row <- fmaf(γ, p, μ)
// μ and p come from ONE function with a fixed rounding order (agr_mu_p), so the write pass rebuilds the
// bits the statistics were taken on. All sums have a fixed order: same rows in, same bits out, on every
// rank. No atomics, no allocation, no synchronisation. Semantics: docs/GAR_SEMANTICS.md "Adaptive
// colluding attacks".
#include "gar_select.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

namespace {

constexpr int kAgrThreads = 256;
constexpr int kAgrWaves = kAgrThreads / 64;
constexpr int kAgrMaxGrid = 4096;   // the combine kernels' cap

// 8 coordinates of a row from element x: one 16-byte load when the launch is aligned (vec) and the
// lane owns a whole vector, single elements otherwise; coordinates past nv read as 0.
template <int DT>
__device__ __forceinline__ void agr_load(const void* row, int64_t x, int nv, int vec, float (&v)[8]) {
  if (vec && nv == 8) {
    load_vec<DT, 8>(row, x, v);
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = c < nv ? load_one<DT>(row, x + c) : 0.f;
  }
}

// μ and p of the lane's 8 coordinates, in a fixed rounding order (no contraction left to the compiler):
// the sum over the rows in row order, one division, and for `std` a second sweep over the same lines,
// q = Σ fma(e, e, q) with e = v - μ, σ = sqrt(q / (k - 1)). Coordinates past nv give μ = p = 0.
template <int DT, int PERT>
__device__ __forceinline__ void agr_mu_p(const RowTable& rows, int k, int64_t x, int nv, int vec, float (&mu)[8],
                                         float (&p)[8]) {
#pragma clang fp contract(off)
  float s[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) s[c] = 0.f;
  int j = 0;
  for (; j + 4 <= k; j += 4) {   // four row loads in flight, the sums in row order all the same
    float v0[8], v1[8], v2[8], v3[8];
    agr_load<DT>(rows.p[j], x, nv, vec, v0);
    agr_load<DT>(rows.p[j + 1], x, nv, vec, v1);
    agr_load<DT>(rows.p[j + 2], x, nv, vec, v2);
    agr_load<DT>(rows.p[j + 3], x, nv, vec, v3);
#pragma unroll
    for (int c = 0; c < 8; ++c) s[c] = (((s[c] + v0[c]) + v1[c]) + v2[c]) + v3[c];
  }
  for (; j < k; ++j) {
    float v[8];
    agr_load<DT>(rows.p[j], x, nv, vec, v);
#pragma unroll
    for (int c = 0; c < 8; ++c) s[c] = s[c] + v[c];
  }
  const float kf = static_cast<float>(k);
#pragma unroll
  for (int c = 0; c < 8; ++c) mu[c] = s[c] / kf;
  if constexpr (PERT == kAgrStd) {
    float q[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) q[c] = 0.f;
    if (k > 1) {
      for (j = 0; j + 4 <= k; j += 4) {
        float v0[8], v1[8], v2[8], v3[8];
        agr_load<DT>(rows.p[j], x, nv, vec, v0);
        agr_load<DT>(rows.p[j + 1], x, nv, vec, v1);
        agr_load<DT>(rows.p[j + 2], x, nv, vec, v2);
        agr_load<DT>(rows.p[j + 3], x, nv, vec, v3);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float e0 = v0[c] - mu[c], e1 = v1[c] - mu[c], e2 = v2[c] - mu[c], e3 = v3[c] - mu[c];
          q[c] = __builtin_fmaf(e3, e3, __builtin_fmaf(e2, e2, __builtin_fmaf(e1, e1, __builtin_fmaf(e0, e0, q[c]))));
        }
      }
      for (; j < k; ++j) {
        float v[8];
        agr_load<DT>(rows.p[j], x, nv, vec, v);
#pragma unroll
        for (int c = 0; c < 8; ++c) { const float e = v[c] - mu[c]; q[c] = __builtin_fmaf(e, e, q[c]); }
      }
    }
    const float km1 = static_cast<float>(k > 1 ? k - 1 : 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) p[c] = -sqrtf(q[c] / km1);
  } else if constexpr (PERT == kAgrUv) {
#pragma unroll
    for (int c = 0; c < 8; ++c) p[c] = -mu[c];
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) p[c] = mu[c] > 0.f ? -1.f : (mu[c] < 0.f ? 1.f : 0.f);
  }
}

// v of the lane that the DPP control CTRL pairs with this one (all 64 lanes active)
template <int CTRL> __device__ __forceinline__ double agr_dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// Σ over the wave in a fixed pairing, as gar_select.hpp's wave_sum_dpp: four steps inside a row of 16 lanes
// through DPP, two across rows through the LDS crossbar. One per estimate row and trip of the statistics
// pass, so the DPP steps matter here.
__device__ __forceinline__ double agr_wave_sum(double v) {
  v += agr_dpp_f64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += agr_dpp_f64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += agr_dpp_f64<0x141>(v);   // row_half_mirror
  v += agr_dpp_f64<0x140>(v);   // row_mirror
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// The loop of both streaming passes: workgroup b takes the 2048-coordinate tiles b, b + grid, ... of
// [lo, hi); every lane of a workgroup makes the same number of trips (the wave sums need all lanes), a
// lane past the end carries nv = 0 and touches no memory.
template <int DT, int PERT>
__global__ __launch_bounds__(kAgrThreads) void k_agr_stats(RowTable rows, int k, int64_t lo, int64_t hi, int vec,
                                                           double* __restrict__ partials) {
  __shared__ double acc[kAgrWaves][kMaxRows + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = lane; t <= k; t += 64) acc[wave][t] = 0.0;
  __syncthreads();
  const int64_t n = hi - lo;
  const int64_t tile = static_cast<int64_t>(kAgrThreads) * 8;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * tile; base < n; base += static_cast<int64_t>(gridDim.x) * tile) {
    const int64_t rel = base + static_cast<int64_t>(threadIdx.x) * 8;
    const int nv = rel >= n ? 0 : (n - rel >= 8 ? 8 : static_cast<int>(n - rel));
    const int64_t x = lo + rel;
    float mu[8], p[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { mu[c] = 0.f; p[c] = 0.f; }
    if (nv > 0) agr_mu_p<DT, PERT>(rows, k, x, nv, vec, mu, p);
    float cc = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) cc = fmaf(p[c], p[c], cc);
    const double cw = agr_wave_sum(static_cast<double>(cc));
    if (lane == 0) acc[wave][k] += cw;
    int i = 0;
    for (; i + 4 <= k; i += 4) {   // four rows' loads and wave sums in flight
      float t[4] = {0.f, 0.f, 0.f, 0.f};
      if (nv > 0) {
        float v0[8], v1[8], v2[8], v3[8];
        agr_load<DT>(rows.p[i], x, nv, vec, v0);
        agr_load<DT>(rows.p[i + 1], x, nv, vec, v1);
        agr_load<DT>(rows.p[i + 2], x, nv, vec, v2);
        agr_load<DT>(rows.p[i + 3], x, nv, vec, v3);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          t[0] = fmaf(p[c], mu[c] - v0[c], t[0]);
          t[1] = fmaf(p[c], mu[c] - v1[c], t[1]);
          t[2] = fmaf(p[c], mu[c] - v2[c], t[2]);
          t[3] = fmaf(p[c], mu[c] - v3[c], t[3]);
        }
      }
      double bw[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) bw[r] = agr_wave_sum(static_cast<double>(t[r]));
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[wave][i + r] += bw[r];
      }
    }
    for (; i < k; ++i) {
      float t = 0.f;
      if (nv > 0) {
        float v[8];
        agr_load<DT>(rows.p[i], x, nv, vec, v);
#pragma unroll
        for (int c = 0; c < 8; ++c) t = fmaf(p[c], mu[c] - v[c], t);
      }
      const double bw = agr_wave_sum(static_cast<double>(t));
      if (lane == 0) acc[wave][i] += bw;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t <= k; t += blockDim.x)
    partials[static_cast<int64_t>(blockIdx.x) * (k + 1) + t] = ((acc[0][t] + acc[1][t]) + acc[2][t]) + acc[3][t];
}

template <int DT, int PERT>
__global__ __launch_bounds__(kAgrThreads) void k_agr_write(RowTable rows, int k, int P, int64_t lo, int64_t hi, int vec,
                                                           const float* __restrict__ gamma) {
  const float g = gamma[0];
  const int64_t n = hi - lo;
  const int64_t tile = static_cast<int64_t>(kAgrThreads) * 8;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * tile; base < n; base += static_cast<int64_t>(gridDim.x) * tile) {
    const int64_t rel = base + static_cast<int64_t>(threadIdx.x) * 8;
    if (rel >= n) continue;
    const int nv = n - rel >= 8 ? 8 : static_cast<int>(n - rel);
    const int64_t x = lo + rel;
    float mu[8], p[8], o[8];
    agr_mu_p<DT, PERT>(rows, k, x, nv, vec, mu, p);   // every row of E at x is read before the first store
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = __builtin_fmaf(g, p[c], mu[c]);
    for (int t = P; t < k; ++t) {
      void* row = const_cast<void*>(rows.p[t]);
      if (vec && nv == 8) {
        store_vec<8>(row, DT, x, o);
      } else {
        for (int c = 0; c < nv; ++c) store_one(row, DT, x + c, o[c]);
      }
    }
  }
}

// Σ_b parts[b][t] in fp64 by one wave, in a fixed order: lane l adds rows l, l + 64, ... in row order,
// then the butterfly of wave_sum_f64. One row comes back bit for bit.
__device__ __forceinline__ double agr_sum_parts(const double* __restrict__ parts, int nparts, int k, int t, int lane) {
  double a = 0.0;
  for (int b = lane; b < nparts; b += 64) a += parts[static_cast<int64_t>(b) * (k + 1) + t];
  return wave_sum_f64(a);
}

__global__ __launch_bounds__(1024) void k_agr_reduce(const double* __restrict__ parts, int nparts, int k,
                                                     double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = wave; t <= k; t += 16) {
    const double a = agr_sum_parts(parts, nparts, k, t, lane);
    if (lane == 0) out[t] = a;
  }
}

// info: [2 + 2k] fp64 = γ, R (Min-Max) or S (Min-Sum), a_0..a_{k-1}, b_0..b_{k-1}
__global__ __launch_bounds__(1024) void k_agr_solve(const float* __restrict__ gram, int np, int k,
                                                    const double* __restrict__ parts, int nparts, int minsum,
                                                    float* __restrict__ gamma32, double* __restrict__ info) {
  extern __shared__ double lds64[];
  double* B = lds64;            // [k + 1] b_i, c
  double* Rs = B + (k + 1);     // [k] Σ_j D_ij
  double* Gi = Rs + k;          // [k] Min-Max: row i's bound on γ; Min-Sum: a_i (NaN: a non-finite input)
  float* D = reinterpret_cast<float*>(Gi + k);   // [k][k + 1]
  float* Mx = D + k * (k + 1);  // [k] max_j D_ij
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, me = threadIdx.x;
  const int pitch = k + 1;
  fill_distances(gram, np, k, D, 0.f);
  for (int t = wave; t <= k; t += 16) {
    const double a = agr_sum_parts(parts, nparts, k, t, lane);
    if (lane == 0) B[t] = a;
  }
  __syncthreads();
  for (int i = wave; i < k; i += 16) {
    const float* row = D + i * pitch;
    double acc = 0.0;
    float mx = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int j = lane + 64 * c;
      if (j < k) { acc += static_cast<double>(row[j]); mx = fmaxf(mx, row[j]); }
    }
    acc = wave_sum_f64(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) { Rs[i] = acc; Mx[i] = mx; }
  }
  __syncthreads();
  // every wave: g = mean_i r_i, R = max_ij D_ij, S = max_i Σ_j D_ij (the same bits on every wave)
  const double kd = static_cast<double>(k);
  const double g = wave_dot(Rs, nullptr, k, lane) / (kd * kd);
  double R = 0.0, S = 0.0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int j = lane + 64 * c;
    if (j < k) { R = fmax(R, static_cast<double>(Mx[j])); S = fmax(S, Rs[j]); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { R = fmax(R, __shfl_xor(R, o, 64)); S = fmax(S, __shfl_xor(S, o, 64)); }
  const double c = B[k];
  if (me < k) {
    const double a = Rs[me] / kd - 0.5 * g, b = B[me];
    double v;
    if (minsum) {
      v = a;
    } else {
      // the root of γ² c + 2 γ b + a - R = 0 that is >= 0, without the cancellation of -b + sqrt(..) at b > 0
      const double t = fmax(R - a, 0.0), disc = sqrt(b * b + c * t);
      v = b > 0.0 ? t / (b + disc) : (disc - b) / c;
    }
    const bool ok = isfinite(a) && isfinite(b);
    Gi[me] = ok ? v : __builtin_nan("");
    info[2 + me] = a;
    info[2 + k + me] = b;
  }
  __syncthreads();
  if (me == 0) {
    double gam;
    if (minsum) {
      double sa = 0.0;
      for (int i = 0; i < k; ++i) sa += Gi[i];
      gam = sqrt(fmax(S - sa, 0.0) / (kd * c));
    } else {
      gam = static_cast<double>(kInf);
      for (int i = 0; i < k; ++i) gam = Gi[i] < gam ? Gi[i] : (Gi[i] == Gi[i] ? gam : Gi[i]);   // NaN sticks
    }
    const double bound = minsum ? S : R;
    if (!(c > 0.0) || k == 1 || !isfinite(c) || !isfinite(bound) || !isfinite(gam)) gam = 0.0;
    float g32 = static_cast<float>(gam);
    if (!isfinite(g32)) g32 = 0.f;
    gamma32[0] = g32;
    info[0] = gam;
    info[1] = bound;
  }
}

size_t agr_lds_bytes(int k) {
  return static_cast<size_t>(3 * k + 1) * sizeof(double) + static_cast<size_t>(k * (k + 1) + k) * sizeof(float);
}

template <int DT> struct AgrStats {
  static void run(const RowTable& rows, int k, int pert, int64_t lo, int64_t hi, int vec, double* partials, int grid,
                  hipStream_t s) {
    if (pert == kAgrStd)
      hipLaunchKernelGGL((k_agr_stats<DT, kAgrStd>), dim3(grid), dim3(kAgrThreads), 0, s, rows, k, lo, hi, vec, partials);
    else if (pert == kAgrUv)
      hipLaunchKernelGGL((k_agr_stats<DT, kAgrUv>), dim3(grid), dim3(kAgrThreads), 0, s, rows, k, lo, hi, vec, partials);
    else
      hipLaunchKernelGGL((k_agr_stats<DT, kAgrSgn>), dim3(grid), dim3(kAgrThreads), 0, s, rows, k, lo, hi, vec, partials);
  }
};

template <int DT> struct AgrWrite {
  static void run(const RowTable& rows, int k, int P, int pert, int64_t lo, int64_t hi, int vec, const float* gamma,
                  int grid, hipStream_t s) {
    if (pert == kAgrStd)
      hipLaunchKernelGGL((k_agr_write<DT, kAgrStd>), dim3(grid), dim3(kAgrThreads), 0, s, rows, k, P, lo, hi, vec, gamma);
    else if (pert == kAgrUv)
      hipLaunchKernelGGL((k_agr_write<DT, kAgrUv>), dim3(grid), dim3(kAgrThreads), 0, s, rows, k, P, lo, hi, vec, gamma);
    else
      hipLaunchKernelGGL((k_agr_write<DT, kAgrSgn>), dim3(grid), dim3(kAgrThreads), 0, s, rows, k, P, lo, hi, vec, gamma);
  }
};

// whether every lane's 8-coordinate group of every row starts on a 16-byte boundary
int agr_vec(const RowTable& rows, int k, int64_t lo, int dt) {
  const int64_t esz = dtype_size(dt);
  for (int j = 0; j < k; ++j)
    if ((reinterpret_cast<uintptr_t>(rows.p[j]) + static_cast<uintptr_t>(lo * esz)) % 16 != 0) return 0;
  return 1;
}

}  // namespace

int agr_grid(int64_t count) {
  int64_t g = (count + kAgrThreads * 8 - 1) / (kAgrThreads * 8);
  if (g < 1) g = 1;
  if (g > kAgrMaxGrid) g = kAgrMaxGrid;
  return static_cast<int>(g);
}

void agr_stats(const RowTable& rows, int k, int64_t lo, int64_t hi, int dt, int pert, double* partials,
               hipStream_t stream) {
  by_dtype<AgrStats>(dt, rows, k, pert, lo, hi, agr_vec(rows, k, lo, dt), partials, agr_grid(hi - lo), stream);
}

void agr_reduce(const double* parts, int nparts, int k, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_agr_reduce, dim3(1), dim3(1024), 0, stream, parts, nparts, k, out);
}

void agr_solve(const float* gram_in, int np, int k, const double* parts, int nparts, bool minsum, float* gamma,
               double* info, hipStream_t stream) {
  launch_select<k_agr_solve>(1, agr_lds_bytes(k), stream, gram_in, np, k, parts, nparts, minsum ? 1 : 0, gamma, info);
}

void agr_write(const RowTable& rows, int k, int P, int64_t lo, int64_t hi, int dt, int pert, const float* gamma,
               hipStream_t stream) {
  if (P >= k || hi <= lo) return;
  by_dtype<AgrWrite>(dt, rows, k, P, pert, lo, hi, agr_vec(rows, k, lo, dt), gamma, agr_grid(hi - lo), stream);
}

}  // namespace gpu
}  // namespace garfield

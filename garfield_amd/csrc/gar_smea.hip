// SMEA, smallest maximum eigenvalue averaging (Allouah, Guerraoui, Gupta, Pinot, Stephan, ICML 2023), on the
// Gram matrix: among the C(n, k) subsets of k = n - f rows, the one whose empirical covariance has the
// smallest top eigenvalue; the result is that subset's mean.
//
// It is Brute's enumeration (gar_gram.hip k_brute_search: k-bit masks in increasing numeric order, the
// combinatorial-number-system unrank, Gosper steps, a (score bits << 32) | rank key reduced by atomicMin)
// with the score of the DnC selection (gar_dnc.hip): the top eigenvalue of (1/k) Σ (x_i - μ)(x_i - μ)ᵀ over
// the members equals that of K_S / k with K_S = -½ J D_S J, D_S the members' k x k block of the squared
// distances, and comes from a fixed number of power rounds on it. Nothing outside the Gram is touched.
// Semantics: docs/GAR_SEMANTICS.md "SMEA".
//
// A subset costs iters · k² multiply-adds, so a subset is a group of G lanes (G = 16, 32 or 64, the
// smallest >= k), not a thread: 64 / G subsets advance side by side in a wave. Lane p < k owns member p: it
// gathers its row of D_S (k fp32 values from the workgroup's LDS copy of D, pitch 65) into registers once
// per subset, and a round's matvec runs from those. The round's centred vector goes through a per-wave
// LDS vector (one ds_write_b64, then k broadcast ds_read_b64 at 2 LDS cycles each; ds_bpermute would
// take two 32-bit permutes per entry, twice the LDS cycles): a wave's DS operations execute in order, so
// no workgroup barrier is needed. Every sum is fp64, reduced over the group by DPP inside a 16-lane row
// and by the cross-row steps of wave_sum_dpp only for G > 16. The two means of a round multiply
// by 1 / k instead of dividing (the oracle divides; the difference is an fp64 rounding, far below the fp32
// score; measured, it saved 4 % at (n, f) = (32, 8): a round is about 1100 SIMD cycles per wave, of which
// the matvec's k converts and multiply-adds are a quarter, profiles/r20/smea/). Each group owns a contiguous rank range,
// unranks once and takes Gosper steps; the trip count is the same for every group, a group past its range
// (or past `total`) stays in the instruction stream and is kept out of the minimum, so no cross-lane
// operation or barrier sits under a divergent branch. Workgroup minimum, one atomicMin per workgroup:
// order-independent, hence deterministic; grid and group size depend on (n, f) alone: capturable.
#include "gar_select.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

namespace {

// Σ over a group of G consecutive lanes, the same bits in every lane of the group: wave_sum_dpp cut to G lanes
template <int G> __device__ __forceinline__ double group_sum(double v) {
  v += dpp_f64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0x140>(v);   // row_mirror
  if (G > 16) v += __shfl_xor(v, 16, 64);
  if (G > 32) v += __shfl_xor(v, 32, 64);
  return v;
}

// a wave's LDS writes before, its LDS reads after: the DS queue keeps the order, the compiler must too
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G>
__global__ __launch_bounds__(256) void k_smea_search(const float* __restrict__ gram, int np, int n, int k, int iters,
                                                     unsigned long long total, unsigned long long per,
                                                     unsigned long long* __restrict__ best) {
  __shared__ float D[64 * 65];
  __shared__ double Vec[256];   // slot t: the centred vector's entry of thread t's member
  __shared__ unsigned long long wbest[4];
  // distances as every selection builds them: clamped at 0, non-finite kept as +inf ("invalid"), diagonal 0
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e / n, j = e % n;
    float v = 0.f;
    if (i != j) {
      v = gram[i * np + i] + gram[j * np + j] - 2.f * gram[i * np + j];
      if (!isfinite(v)) v = kInf;
      v = fmaxf(v, 0.f);
    }
    D[i * 65 + j] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int p = threadIdx.x & (G - 1);        // position in the group = the member this lane owns
  const int gbase = threadIdx.x & ~(G - 1);   // the group's first slot of Vec
  const bool live = p < k;
  const double kd = static_cast<double>(k);
  const double ik = 1.0 / kd;   // the means of a round multiply by 1 / k
  const unsigned long long group = static_cast<unsigned long long>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  const unsigned long long low = k >= 64 ? ~0ull : (1ull << k) - 1ull;   // a valid mask for a group out of range
  const unsigned long long gmask = G >= 64 ? ~0ull : (1ull << G) - 1ull;
  const unsigned long long r0 = group * per;
  unsigned long long r1 = r0 + per;
  if (r1 > total) r1 = total;
  unsigned long long mask = r0 < total ? subset_unrank(r0, n, k) : low;
  unsigned long long my = ~0ull;
  for (unsigned long long step = 0; step < per; ++step) {   // the same trip count in every group
    const unsigned long long rank = r0 + step;
    const bool active = rank < r1;
    // this lane's member: the p-th set bit (dead lanes take member 0 and are masked out of every sum)
    int me = 0;
    unsigned long long mi = mask;
#pragma unroll
    for (int q = 0; q < G; ++q) {
      if (q < k) {
        const int j = __builtin_ctzll(mi);
        mi &= mi - 1ull;
        if (q == p) me = j;
      }
    }
    // its row of D_S, in member order
    float row[G];
    bool bad = false;
    double rs = 0.0;
    mi = mask;
#pragma unroll
    for (int q = 0; q < G; ++q) {
      row[q] = 0.f;
      if (q < k) {
        const int j = __builtin_ctzll(mi);
        mi &= mi - 1ull;
        row[q] = D[me * 65 + j];
        bad = bad || row[q] == kInf;
        rs += static_cast<double>(row[q]);
      }
    }
    const bool gbad = ((__ballot(bad && live) >> (lane & ~(G - 1))) & gmask) != 0ull;   // a non-finite pair
    // r_p = mean_q D_pq, g = mean r, the start: the column of K_S at the member of largest κ_p = r_p - g/2
    const double r = live ? rs / kd : 0.0;
    const double g = group_sum<G>(r) / kd;
    double kb = live ? r - 0.5 * g : -static_cast<double>(kInf);
    int star = p;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
      const double ko = __shfl_xor(kb, o, 64);
      const int so = __shfl_xor(star, o, 64);
      if (ko > kb || (ko == kb && so < star)) { kb = ko; star = so; }   // ties: the lowest position
    }
    star &= G - 1;
    const double rstar = __shfl(r, star, G);
    const int mstar = __shfl(me, star, G);
    double b = live ? -0.5 * (static_cast<double>(D[me * 65 + mstar]) - r - rstar + g) : 0.0;
    double u = 0.0;
    for (int it = 0; it < iters; ++it) {
      const double nu = sqrt(group_sum<G>(b * b));
      u = nu > 0.0 ? b / nu : 0.0;
      const double c = group_sum<G>(u) * ik;
      Vec[threadIdx.x] = live ? u - c : 0.0;
      wave_lds_sync();
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < G; ++q)
        if (q < k) t += static_cast<double>(row[q]) * Vec[gbase + q];
      wave_lds_sync();
      t = live ? t : 0.0;
      const double tm = group_sum<G>(t) * ik;
      b = live ? -0.5 * (t - tm) : 0.0;
    }
    const double lam = group_sum<G>(u * b) / kd;
    float s = static_cast<float>(lam);
    if (!(s >= 0.f)) s = s < 0.f ? 0.f : kInf;   // negative: 0; NaN: +inf
    if (gbad) s = kInf;
    const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(s)) << 32) | rank;
    if (active && key < my) my = key;
    // Gosper: the next k-bit mask in numeric order (the lowest set bit is a power of two: a shift divides)
    const unsigned long long c = mask & (~mask + 1ull);
    const unsigned long long rr = mask + c;
    mask = rank + 1ull < r1 ? ((((rr ^ mask) >> 2) >> __builtin_ctzll(c)) | rr) : low;
  }
  // wave min, workgroup min, one atomic per workgroup (order-independent => deterministic)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(my, o, 64);
    my = other < my ? other : my;
  }
  if (lane == 0) wbest[threadIdx.x >> 6] = my;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = wbest[0];
    for (int w = 1; w < 4; ++w) m = wbest[w] < m ? wbest[w] : m;
    atomicMin(best, m);
  }
}

unsigned long long subset_count(int n, int k) {
  if (k > n - k) k = n - k;
  unsigned long long r = 1;
  for (int i = 1; i <= k; ++i) r = r * static_cast<unsigned long long>(n - k + i) / static_cast<unsigned long long>(i);
  return r;
}

template <int G>
void launch_search(const float* gram, int np, int n, int k, int iters, unsigned long long total,
                   unsigned long long* best, hipStream_t stream) {
  // at most 1024 workgroups of four waves: one round of the device for G = 16 and 32 (86 and 120 VGPRs, five
  // and four waves per SIMD), two rounds for G = 64 (195 VGPRs, two waves per SIMD). A subset costs far
  // more than the unrank (n binomials), so small problems spread out to one subset per group
  const unsigned long long groups_max = 1024ull * (256 / G);
  unsigned long long per = (total + groups_max - 1) / groups_max;
  if (per < 1) per = 1;
  const unsigned long long groups = (total + per - 1) / per;
  const unsigned int blocks = static_cast<unsigned int>((groups + (256 / G) - 1) / (256 / G));
  hipLaunchKernelGGL(k_smea_search<G>, dim3(blocks), dim3(256), 0, stream, gram, np, n, k, iters, total, per, best);
}

}  // namespace

void smea_select(const float* gram_in, int np, int n, int f, int iters, unsigned long long* best, float* weights,
                 float* scores, hipStream_t stream) {
  const int k = n - f;
  const unsigned long long total = subset_count(n, k);   // the caller keeps it below 2^32: the key's rank word
  hipLaunchKernelGGL(k_subset_init<>, dim3(1), dim3(1), 0, stream, best);
  if (k <= 16) launch_search<16>(gram_in, np, n, k, iters, total, best, stream);
  else if (k <= 32) launch_search<32>(gram_in, np, n, k, iters, total, best, stream);
  else launch_search<64>(gram_in, np, n, k, iters, total, best, stream);
  hipLaunchKernelGGL(k_subset_finalize<true>, dim3(1), dim3(64), 0, stream, best, n, k, weights, scores);
}

}  // namespace gpu
}  // namespace garfield

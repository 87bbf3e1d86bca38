// Worker-side momentum (docs/GAR_SEMANTICS.md "Worker momentum"): every logical worker sends its
// momentum m_i, not its gradient g_i. One streaming pass over coordinates [lo, hi) of the k exchange
// rows, in place, before any simulated attack and before anything leaves the rank:
//   first step:   m <- g                         later:   m <- fmaf(beta, m, omega * g)
//   row <- cast(m)   (round-to-nearest-even of the fp32 state value just stored)
// with g the row's value widened to fp32 and omega = 1 - beta rounded once to fp32 on the host. A
// non-finite g stays in the row and leaves the state as it was: one bad step does not poison a
// worker's state for good. cpu::worker_momentum (gar_cpu.cpp) is the same formula: equal inputs give
// equal bits.
//
// Pure memory traffic, 12 B per element with 16-bit rows (2 + 4 read, 4 + 2 written). The row of a
// workgroup is blockIdx.y; each lane takes 8 consecutive coordinates per trip (one 16-B row load, two
// 16-B state loads, two 16-B state stores, one 16-B row store; 4 coordinates with fp32 rows) and
// issues the loads of two trips before the first use, in a grid-stride loop over the range. Row base
// offsets are 64-bit (k * ld passes 2^31); offsets inside a row are 32-bit. [lo, hi) and the
// alignment of the two buffers are arbitrary: a scalar head runs up to the first coordinate at which
// both the row and the state are 16-byte aligned, a scalar tail after the last whole vector; a row
// whose two buffers never align together runs scalar altogether. Nothing outside [lo, hi) is read or
// written. No atomics, no LDS, plain vector stores: deterministic by construction. beta, omega and
// `first` are kernel arguments by value, so a captured launch replays the values it was captured with.
#include "gar_device.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

namespace {

// g finite: the new state (g itself on the first step); else the old state.
__device__ __forceinline__ float mom_next(float g, float m, float beta, float omega, bool first) {
  if (!isfinite(g)) return m;
  return first ? g : __fmaf_rn(beta, m, __fmul_rn(omega, g));
}

template <int DT> struct RowVec;          // one 16-byte vector of the exchange row
template <> struct RowVec<kF32> { static constexpr int kN = 4; };
template <> struct RowVec<kBF16> { static constexpr int kN = 8; };
template <> struct RowVec<kF16> { static constexpr int kN = 8; };

template <int DT> __device__ __forceinline__ uint16_t cast16(float v) {
  return DT == kBF16 ? f_to_bf16(v) : f_to_f16(v);
}

// One trip's registers: the row vector as loaded and the state.
template <int DT> struct Trip {
  uint4 r;
  float4 m[RowVec<DT>::kN / 4];
};

template <int DT>
__device__ __forceinline__ void trip_load(const void* xr, const float* mr, int x, Trip<DT>& t) {
  constexpr int N = RowVec<DT>::kN;
  if constexpr (DT == kF32) t.r = *reinterpret_cast<const uint4*>(static_cast<const float*>(xr) + x);
  else t.r = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(xr) + x);
#pragma unroll
  for (int q = 0; q < N / 4; ++q) t.m[q] = *reinterpret_cast<const float4*>(mr + x + 4 * q);
}

template <int DT>
__device__ __forceinline__ void trip_store(void* xr, float* mr, int x, const Trip<DT>& t, float beta, float omega,
                                           bool first) {
  constexpr int N = RowVec<DT>::kN;
  const uint32_t w[4] = {t.r.x, t.r.y, t.r.z, t.r.w};
  float m[N];
#pragma unroll
  for (int q = 0; q < N / 4; ++q) { m[4 * q] = t.m[q].x; m[4 * q + 1] = t.m[q].y; m[4 * q + 2] = t.m[q].z; m[4 * q + 3] = t.m[q].w; }
  uint32_t o[4];
  if constexpr (DT == kF32) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float g = __uint_as_float(w[c]);
      m[c] = mom_next(g, m[c], beta, omega, first);
      o[c] = isfinite(g) ? __float_as_uint(m[c]) : w[c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float g0 = cvt16<DT>(w[c] & 0xffffu), g1 = cvt16<DT>(w[c] >> 16);
      m[2 * c] = mom_next(g0, m[2 * c], beta, omega, first);
      m[2 * c + 1] = mom_next(g1, m[2 * c + 1], beta, omega, first);
      const uint32_t lo16 = isfinite(g0) ? cast16<DT>(m[2 * c]) : (w[c] & 0xffffu);
      const uint32_t hi16 = isfinite(g1) ? cast16<DT>(m[2 * c + 1]) : (w[c] >> 16);
      o[c] = lo16 | (hi16 << 16);
    }
  }
#pragma unroll
  for (int q = 0; q < N / 4; ++q)
    *reinterpret_cast<float4*>(mr + x + 4 * q) = make_float4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
  const uint4 ov = make_uint4(o[0], o[1], o[2], o[3]);
  if constexpr (DT == kF32) *reinterpret_cast<uint4*>(static_cast<float*>(xr) + x) = ov;
  else *reinterpret_cast<uint4*>(static_cast<uint16_t*>(xr) + x) = ov;
}

template <int DT>
__device__ __forceinline__ void one(void* xr, float* mr, int x, float beta, float omega, bool first) {
  if constexpr (DT == kF32) {
    float* p = static_cast<float*>(xr) + x;
    const float g = *p;
    if (isfinite(g)) *p = mr[x] = mom_next(g, mr[x], beta, omega, first);
  } else {
    uint16_t* p = static_cast<uint16_t*>(xr) + x;
    const float g = cvt16<DT>(*p);
    if (isfinite(g)) {
      const float m = mom_next(g, mr[x], beta, omega, first);
      mr[x] = m;
      *p = cast16<DT>(m);
    }
  }
}

}  // namespace

// X: row r at X + r * xstride elements; M: row r at M + r * ld floats; 0 <= lo < hi <= ld.
template <int DT>
__global__ __launch_bounds__(256) void k_worker_momentum(void* __restrict__ X, int64_t xstride, float* __restrict__ M,
                                                         int64_t ld, int lo, int hi, float beta, float omega,
                                                         int first_in) {
  constexpr int N = RowVec<DT>::kN;
  constexpr int ESZ = DT == kF32 ? 4 : 2;
  const bool first = first_in != 0;
  const int64_t r = blockIdx.y;
  void* xr = static_cast<char*>(X) + r * xstride * ESZ;
  float* mr = M + r * ld;
  // the scalar head: up to the first coordinate at which the row is 16-byte aligned, if the state is then too
  const int len = hi - lo;
  const uintptr_t xa = reinterpret_cast<uintptr_t>(xr) / ESZ + static_cast<uintptr_t>(lo);   // in elements
  const uintptr_t ma = reinterpret_cast<uintptr_t>(mr) / 4 + static_cast<uintptr_t>(lo);     // in floats
  int head = static_cast<int>((N - xa % N) % N);
  if ((ma + head) % 4 != 0) head = len;   // the two buffers never align together: scalar altogether
  if (head > len) head = len;
  const int nvec = (len - head) / N;
  const int v0 = lo + head;               // the first vector's coordinate
  const int t0 = v0 + nvec * N;           // the scalar tail's
  const int stride = gridDim.x * blockDim.x;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += 2 * stride) {
    const int u = v + stride;             // the second trip: its loads leave before the first trip's use
    Trip<DT> a, b;
    trip_load<DT>(xr, mr, v0 + v * N, a);
    if (u < nvec) trip_load<DT>(xr, mr, v0 + u * N, b);
    trip_store<DT>(xr, mr, v0 + v * N, a, beta, omega, first);
    if (u < nvec) trip_store<DT>(xr, mr, v0 + u * N, b, beta, omega, first);
  }
  const int nscalar = head + (hi - t0);
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < nscalar; s += stride)
    one<DT>(xr, mr, s < head ? lo + s : t0 + (s - head), beta, omega, first);
}

// Workgroups of a launch, all rows together. 4096 is the cap of the combine + update kernel
// (combine_grid, gar_combine.hip), whose 5.3 TB/s at d = 23.5M bf16 (README "Kernels") was measured
// with it; this pass's own rate at that cap: profiles/r11/worker_momentum/.
constexpr int kWorkerMomGrid = 4096;

void worker_momentum(void* X, int dt, int64_t xstride, float* M, int64_t ld, int k, int64_t lo, int64_t hi, float beta,
                     float omega, bool first, hipStream_t stream) {
  if (k <= 0 || hi <= lo) return;
  const int n = dt == kF32 ? 4 : 8;
  const int64_t nvec = (hi - lo + n - 1) / n;
  int64_t gx = (nvec + 255) / 256;
  const int64_t cap = kWorkerMomGrid / k > 1 ? kWorkerMomGrid / k : 1;
  if (gx > cap) gx = cap;
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(k));
  const int l = static_cast<int>(lo), h = static_cast<int>(hi), f = first ? 1 : 0;
  if (dt == kF32)
    hipLaunchKernelGGL(k_worker_momentum<kF32>, grid, dim3(256), 0, stream, X, xstride, M, ld, l, h, beta, omega, f);
  else if (dt == kBF16)
    hipLaunchKernelGGL(k_worker_momentum<kBF16>, grid, dim3(256), 0, stream, X, xstride, M, ld, l, h, beta, omega, f);
  else
    hipLaunchKernelGGL(k_worker_momentum<kF16>, grid, dim3(256), 0, stream, X, xstride, M, ld, l, h, beta, omega, f);
}

}  // namespace gpu
}  // namespace garfield

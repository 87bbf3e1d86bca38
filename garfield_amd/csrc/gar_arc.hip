// Adaptive robust clipping (ARC; Allouah et al., "Boosting Robustness by Clipping Gradients in
// Distributed Learning") in front of a rule. Semantics: docs/GAR_SEMANTICS.md "Adaptive robust clipping".
//
// The k = (2 f (n - f)) / n rows of largest norm are scaled down to the norm of the (k + 1)-th largest.
// The decision needs the squared norms alone, the Gram's diagonal, and clipping is linear per row:
//   k_arc_scale  one workgroup per problem: the threshold C² by rank counting on (norm descending, index
//                ascending), the scales c_i = sqrt(C² / s_i) (1 on the rows that are not clipped), the list
//                of the clipped rows and, when asked for, the clipped rows' Gram G'_ij = (c_i c_j) G_ij, on
//                which the selections run unchanged;
//   k_arc_fold   w_j = c_j a_j: the rule's weights over the clipped rows as weights over the ORIGINAL rows,
//                which the combine kernels consume (no pass over the d-length rows);
//   k_arc_apply  only for the coordinate-wise rules, which have no weights to fold into: row <- cast(c · row)
//                in place on coordinates [lo, hi) of the clipped rows only.
// The scales and the list stay on the device: every launch can be captured, the grid of k_arc_apply is
// sized by the host-known bound k and a workgroup past the device's count leaves after one uniform load.
// fp64 `/`, `sqrt` and products, each rounded once to fp32: bit-equal to the fp64 oracle on the same Gram.
//
// k_arc_apply is pure memory traffic (read + write of the clipped rows) and follows worker_mom.hip: the
// row of a workgroup is blockIdx.y's entry of the list, each lane takes one 16-byte vector per trip (8
// coordinates, 4 with fp32 rows) and issues the loads of two trips before the first use, in a grid-stride
// loop; row bases are 64-bit pointers of the RowTable, offsets inside a row 32-bit; a scalar head runs up to
// the row's first 16-byte aligned coordinate and a scalar tail after the last whole vector. Nothing outside
// [lo, hi) and nothing in an unclipped row is read for writing or written. No atomics, no LDS, plain vector
// stores: deterministic by construction.
#include "gar_device.hpp"

namespace garfield {
namespace gpu {

using namespace dev;

// gram [batch][np][np] -> scales [batch][n], clip_rows [batch][n + 1] (count, the clipped rows ascending,
// -1 on the rest), gout [batch][np][np] (nullptr: not written; may be gram itself: every entry is read
// and written by one thread, the diagonal is read before the first barrier).
__global__ __launch_bounds__(1024) void k_arc_scale(const float* gram, int np, int n, int k,
                                                    float* __restrict__ scales, int* __restrict__ clip_rows,
                                                    float* gout) {
  __shared__ float key[kMaxRows];     // s_i, +inf where non-finite
  __shared__ float cs[kMaxRows];      // c_i
  __shared__ int clipped[kMaxRows];
  __shared__ float c2;
  gram += static_cast<int64_t>(blockIdx.x) * np * np;
  if (gout) gout += static_cast<int64_t>(blockIdx.x) * np * np;
  scales += static_cast<int64_t>(blockIdx.x) * n;
  clip_rows += static_cast<int64_t>(blockIdx.x) * (n + 1);
  const int i = threadIdx.x;
  float s = 0.f;
  if (i < n) {
    s = gram[i * np + i];
    key[i] = isfinite(s) ? s : kInf;
  }
  __syncthreads();
  // the row at position k of the order (s descending, index ascending); ranks are counted, not sorted
  if (i < n) {
    const float ki = key[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float kj = key[j];
      rank += (kj > ki) || (kj == ki && j < i);
    }
    if (rank == k) c2 = ki;
  }
  __syncthreads();
  if (i < n) {
    const float t = c2;
    float c = 1.f;
    if (isfinite(s) && t != kInf && s > t) c = static_cast<float>(sqrt(static_cast<double>(t) / static_cast<double>(s)));
    cs[i] = c;
    clipped[i] = c != 1.f;
    scales[i] = c;
  }
  __syncthreads();
  if (i < n) {
    int before = 0, total = 0;
    for (int j = 0; j < n; ++j) {
      before += j < i ? clipped[j] : 0;
      total += clipped[j];
    }
    if (clipped[i]) clip_rows[1 + before] = i;
    if (i >= total) clip_rows[1 + i] = -1;
    if (i == 0) clip_rows[0] = total;
  }
  if (!gout) return;
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int r = e / n, c = e % n;
    const float g = gram[r * np + c];
    const double cc = static_cast<double>(cs[r]) * static_cast<double>(cs[c]);
    gout[r * np + c] = cc == 1.0 ? g : static_cast<float>(cc * static_cast<double>(g));
  }
}

__global__ __launch_bounds__(128) void k_arc_fold(const float* __restrict__ a, const float* __restrict__ scales, int n,
                                                  float* __restrict__ w) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * n;
  const int j = threadIdx.x;
  if (j < n) w[base + j] = static_cast<float>(static_cast<double>(scales[base + j]) * static_cast<double>(a[base + j]));
}

namespace {

template <int DT> struct ArcVec { static constexpr int kN = DT == kF32 ? 4 : 8; };

template <int DT> __device__ __forceinline__ uint4 arc_load(const void* xr, int x) {
  if constexpr (DT == kF32) return *reinterpret_cast<const uint4*>(static_cast<const float*>(xr) + x);
  else return *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(xr) + x);
}

// one fp32 multiply per element, rounded to the row's dtype to nearest even
template <int DT> __device__ __forceinline__ void arc_store(void* xr, int x, const uint4& r, float c) {
#pragma clang fp contract(off)
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  uint32_t o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if constexpr (DT == kF32) {
      o[q] = __float_as_uint(c * __uint_as_float(w[q]));
    } else {
      const float v0 = c * cvt16<DT>(w[q] & 0xffffu), v1 = c * cvt16<DT>(w[q] >> 16);
      if constexpr (DT == kBF16) o[q] = pack_bf16x2(v0, v1);
      else o[q] = static_cast<uint32_t>(f_to_f16(v0)) | (static_cast<uint32_t>(f_to_f16(v1)) << 16);
    }
  }
  const uint4 ov = make_uint4(o[0], o[1], o[2], o[3]);
  if constexpr (DT == kF32) *reinterpret_cast<uint4*>(static_cast<float*>(xr) + x) = ov;
  else *reinterpret_cast<uint4*>(static_cast<uint16_t*>(xr) + x) = ov;
}

template <int DT> __device__ __forceinline__ void arc_one(void* xr, int x, float c) {
#pragma clang fp contract(off)
  if constexpr (DT == kF32) {
    float* p = static_cast<float*>(xr) + x;
    *p = c * *p;
  } else {
    uint16_t* p = static_cast<uint16_t*>(xr) + x;
    const float v = c * cvt16<DT>(*p);
    *p = DT == kBF16 ? f_to_bf16(v) : f_to_f16(v);
  }
}

}  // namespace

// rows: the n exchange rows; clip_rows / scales: k_arc_scale's outputs; 0 <= lo < hi < 2^31 inside every row.
template <int DT>
__global__ __launch_bounds__(256) void k_arc_apply(RowTable rows, int n, const int* __restrict__ clip_rows,
                                                   const float* __restrict__ scales, int lo, int hi) {
  constexpr int N = ArcVec<DT>::kN;
  constexpr int ESZ = DT == kF32 ? 4 : 2;
  if (static_cast<int>(blockIdx.y) >= clip_rows[0]) return;   // fewer rows clipped than the host's bound k
  const int r = clip_rows[1 + blockIdx.y];
  if (r < 0 || r >= n) return;            // a list k_arc_scale did not write: touch nothing
  const float c = scales[r];
  void* xr = const_cast<void*>(rows.p[r]);
  // the scalar head: up to the first coordinate at which the row is 16-byte aligned
  const int len = hi - lo;
  const uintptr_t xa = reinterpret_cast<uintptr_t>(xr) / ESZ + static_cast<uintptr_t>(lo);   // in elements
  int head = static_cast<int>((N - xa % N) % N);
  if (head > len) head = len;
  const int nvec = (len - head) / N;
  const int v0 = lo + head;               // the first vector's coordinate
  const int t0 = v0 + nvec * N;           // the scalar tail's
  const int stride = gridDim.x * blockDim.x;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += 2 * stride) {
    const int u = v + stride;             // the second trip: its load leaves before the first trip's use
    const uint4 a = arc_load<DT>(xr, v0 + v * N);
    uint4 b = a;
    if (u < nvec) b = arc_load<DT>(xr, v0 + u * N);
    arc_store<DT>(xr, v0 + v * N, a, c);
    if (u < nvec) arc_store<DT>(xr, v0 + u * N, b, c);
  }
  const int nscalar = head + (hi - t0);
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < nscalar; s += stride)
    arc_one<DT>(xr, s < head ? lo + s : t0 + (s - head), c);
}

int arc_count(int n, int f) { return static_cast<int>((2 * static_cast<int64_t>(f) * (n - f)) / n); }

void arc_scale(const float* gram, int np, int n, int f, float* scales, int* clip_rows, float* gram_out,
               hipStream_t stream, int batch) {
  hipLaunchKernelGGL(k_arc_scale, dim3(batch), dim3(1024), 0, stream, gram, np, n, arc_count(n, f), scales, clip_rows,
                     gram_out);
}

void arc_fold(const float* a, const float* scales, int n, float* w, hipStream_t stream, int batch) {
  hipLaunchKernelGGL(k_arc_fold, dim3(batch), dim3(128), 0, stream, a, scales, n, w);
}

// Workgroups of a launch, all clipped rows together: the cap of worker_mom.hip and of the combine kernel.
constexpr int kArcApplyGrid = 4096;

void arc_apply(const RowTable& rows, int n, int k, int64_t lo, int64_t hi, int dt, const int* clip_rows, const float* scales,
               hipStream_t stream) {
  if (k <= 0 || hi <= lo) return;
  const int per = dt == kF32 ? 4 : 8;
  const int64_t nvec = (hi - lo + per - 1) / per;
  int64_t gx = (nvec + 255) / 256;
  const int64_t cap = kArcApplyGrid / k > 1 ? kArcApplyGrid / k : 1;
  if (gx > cap) gx = cap;
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(k));
  const int l = static_cast<int>(lo), h = static_cast<int>(hi);
  if (dt == kF32) hipLaunchKernelGGL(k_arc_apply<kF32>, grid, dim3(256), 0, stream, rows, n, clip_rows, scales, l, h);
  else if (dt == kBF16) hipLaunchKernelGGL(k_arc_apply<kBF16>, grid, dim3(256), 0, stream, rows, n, clip_rows, scales, l, h);
  else hipLaunchKernelGGL(k_arc_apply<kF16>, grid, dim3(256), 0, stream, rows, n, clip_rows, scales, l, h);
}

}  // namespace gpu
}  // namespace garfield

// k_nnm_coord, MFMA form: nearest-neighbour mixing followed by a coordinate-wise rule for bf16 / fp16
// rows, n <= 64, without ever storing the mixed rows.
//
// Per coordinate the n mixed values y_i = (1/c) Σ_{j∈S_i} x_j are a GEMM with the 0/1 set matrix:
// C[n x coords] = S[n x n] · G[n x coords]. This is the structure of Bulyan's MFMA tail
// (gar_bulyan_tail.hpp), whose staging and fragment layout are reused: one wave per 64-coordinate
// group, the [n x 64] tile wave-local in LDS (16-byte loads, the next group's in flight), B fragments
// by ds_read_b64_tr_b16, MB x 2 x KS v_mfma_f32_32x32x16, a v_permlane32_swap so that lane =
// coordinate, the scale 1/c in fp32 and the rule in registers (nnm_rule). S is exact in bf16 / fp16
// and built once per workgroup from the two mask words of the sets launch. A non-finite input turns
// 0 · inf into NaN for every set of its coordinate: such groups are listed and their poisoned coordinates
// redone with direct per-set sums from the LDS tile (MFMA columns are independent: the other coordinates
// of the group keep their bits), as is the whole partial last group (d % 64).
#include "gar_nnm_coord.hpp"

namespace garfield {
namespace gpu {
namespace coord {

namespace {

template <int DT, int NP, int MODE>
__global__ __launch_bounds__(256, 2) void k_nnm_coord_mfma(RowTable rows, int n, int64_t ngroups, int last_width, int f,
                                                           const u64* __restrict__ masks, void* out, int out_dt) {
  constexpr int KS = NP <= 16 ? 1 : NP / 16;  // 16-row MFMA k-steps
  constexpr int MB = NP > 32 ? 2 : 1;         // 32-row MFMA blocks of sets
  constexpr int KR = 16 * KS;                 // gradient rows (padded)
  constexpr int KRP = KR + 8;                 // sA pitch (as the Bulyan tail's)
  __shared__ __align__(16) unsigned char tiles[4][KR * kMfmaTailPitch];
  __shared__ __align__(16) uint16_t sA[32 * MB * KRP];
  __shared__ const void* sptr[KR];
  __shared__ uint64_t smask[NP];
  __shared__ int64_t sbad[4][kTailBadSlots];
  __shared__ int sbadn[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  {  // the set matrix: row k = S_k (n <= 64: the first mask word), zero rows beyond n
    const uint16_t one = DT == kBF16 ? 0x3F80 : 0x3C00;
    for (int k = wave; k < 32 * MB; k += 4) {
      const uint64_t m = k < n ? static_cast<uint64_t>(masks[2 * k]) : 0ull;
      if (lane < KR) sA[k * KRP + lane] = ((m >> lane) & 1ull) ? one : 0;
      if (k < NP && lane == 0) smask[k] = m;
    }
  }
  for (int j = threadIdx.x; j < KR; j += blockDim.x) sptr[j] = rows.p[j < n ? j : 0];
  if (threadIdx.x < 4) sbadn[threadIdx.x] = 0;
  __syncthreads();
  unsigned char* tile = tiles[wave];
  // ds_read_b64_tr_b16 addressing, as in k_bulyan_tail_mfma
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int tr_off = (8 * (g >> 1) + q) * kMfmaTailPitch + (16 * (g & 1) + 4 * p) * 2;
  const int a_off = (lane & 31) * KRP + 8 * (lane >> 5);
  const float inv_c = 1.f / static_cast<float>(n - f);
  bool overflow = false;
  const int64_t gstep = static_cast<int64_t>(gridDim.x) * 4;
  const int64_t gfirst = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  TileRegs<KR> pre;
  if (gfirst < ngroups) tile_load<KR>(pre, sptr, gfirst * 64, lane, n);
  for (int64_t gi = gfirst; gi < ngroups; gi += gstep) {
    asm volatile("" ::: "memory");  // sA is re-read every group: no hoisting into registers
    const int64_t x0 = gi * 64;
    const int nn = opaque_uniform(n), ff = opaque_uniform(f);
    tile_store<KR>(tile, pre, nn, lane);
    if (gi + gstep < ngroups) tile_load<KR>(pre, sptr, (gi + gstep) * 64, lane, nn);  // flies during this group
    f32x16_t acc[MB][2];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.f;
#pragma unroll
    for (int ks_ = 0; ks_ < KS; ++ks_) {
      s16x8_t afrag[MB];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        afrag[mb] = *reinterpret_cast<const s16x8_t*>(&sA[a_off + 32 * mb * KRP + 16 * ks_]);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;
        const unsigned char* base = tile + ks_ * 16 * kMfmaTailPitch + nb * 64 + tr_off;
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base));
        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + 4 * kMfmaTailPitch));
        const s16x8_t bfrag = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb][nb] = mfma32x32x16<DT>(afrag[mb], bfrag, acc[mb][nb]);
      }
    }
    // lane = coordinate: swap the halves so each lane holds the NP set sums of x0 + lane
    float v[NP];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k0 = 32 * mb + (i & 3) + 8 * (i >> 2);
        if (k0 < NP) {
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[mb][0][i]),
                                                           __float_as_uint(acc[mb][1][i]), false, false);
          v[k0] = __uint_as_float(sw[0]);
          v[k0 + 4] = __uint_as_float(sw[1]);
        }
      }
    // chk stays 0 unless a sum is inf / NaN (x * 0 is NaN exactly then): such groups go to the exact pass
    float chk = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      chk = __builtin_fmaf(v[k], 0.f, chk);
      v[k] *= inv_c;
    }
    if (__builtin_amdgcn_ballot_w64(chk != 0.f)) {
      const int slot = sbadn[wave];
      if (slot < kTailBadSlots) {
        if (lane == 0) sbad[wave][slot] = gi;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) sbadn[wave] = slot + 1;
      } else {
        overflow = true;
      }
    }
    store_one(out, out_dt, x0 + lane, nnm_rule<NP, MODE>(v, nn, ff));
  }
  // exact pass: the listed groups (after an overflow of the list: every group of this wave) with direct
  // per-set sums from the LDS tile, plain IEEE: a non-finite member reaches exactly the sets that hold
  // it. Then the partial last group (last_width < 64 coordinates), which is block 0 / wave 0's.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const int nbad = overflow ? 0 : sbadn[wave];
  bool partial_pending = last_width > 0 && gfirst == 0;
  int64_t gi = overflow ? gfirst : 0;
  for (int b = 0;; ++b) {
    int64_t gcur;
    int width = 64;
    if (overflow ? gi < ngroups : b < nbad) {
      gcur = overflow ? gi : sbad[wave][b];
      if (overflow) gi += gstep;
    } else if (partial_pending) {
      gcur = ngroups;
      width = last_width;
      partial_pending = false;
    } else {
      break;
    }
    const int64_t x0 = gcur * 64;
    const int nn = opaque_uniform(n), ff = opaque_uniform(f);
    if (width == 64) {
      stage_tile<DT, KR>(tile, sptr, nn, x0, lane);
    } else {  // partial group: per-column loads, columns >= width repeat the first
      const int64_t xs = x0 + (lane < width ? lane : 0);
      for (int j = 0; j < KR; ++j)
        reinterpret_cast<uint16_t*>(tile)[j * (kMfmaTailPitch / 2) + lane] =
            j < nn ? static_cast<const uint16_t*>(sptr[j])[xs] : 0;
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    const uint16_t* col = reinterpret_cast<const uint16_t*>(tile) + lane;
    // MFMA columns are independent: in a listed group only the coordinates that hold a non-finite input
    // were poisoned, and only they are rewritten (the others keep the bits of the MFMA form)
    float poison = 0.f;
    for (int j = 0; j < nn; ++j) poison = __builtin_fmaf(cvt16<DT>(col[j * (kMfmaTailPitch / 2)]), 0.f, poison);
    const bool rewrite = width < 64 || poison != 0.f;
    float v[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      v[k] = kInf;
      if (k < nn) {
        uint64_t m = uniform64(lds_volatile(smask[k]));
        float s = 0.f;
#pragma clang loop unroll(disable)
        while (m) {
          s += cvt16<DT>(col[__builtin_ctzll(m) * (kMfmaTailPitch / 2)]);
          m &= m - 1;
        }
        v[k] = s * inv_c;
      }
    }
    const float r = nnm_rule<NP, MODE>(v, nn, ff);
    if (lane < width && rewrite) store_one(out, out_dt, x0 + lane, r);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // tile reads done before the next group is staged
  }
}

template <int DT, int MODE>
void launch_np(const RowTable& rows, int n, int64_t d, int f, const u64* masks, void* out, int out_dt, hipStream_t s) {
  const int64_t groups = d / 64;
  const int last = static_cast<int>(d - groups * 64);
  int64_t g = (groups + 3) / 4;
  const int64_t cap = tail_grid_cap(4096);
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  const dim3 grid(static_cast<unsigned>(g)), block(256);
#define GARFIELD_NNM_MFMA(NP) \
  hipLaunchKernelGGL((k_nnm_coord_mfma<DT, NP, MODE>), grid, block, 0, s, rows, n, groups, last, f, masks, out, out_dt)
  if (n <= 8) GARFIELD_NNM_MFMA(8);
  else if (n <= 16) GARFIELD_NNM_MFMA(16);
  else if (n <= 32) GARFIELD_NNM_MFMA(32);
  else GARFIELD_NNM_MFMA(64);
#undef GARFIELD_NNM_MFMA
}

}  // namespace

void launch_nnm_coord_mfma(const RowTable& rows, int n, int64_t d, int dt, int mode, int f, const u64* masks,
                           void* out, int out_dt, hipStream_t s) {
  if (dt == kBF16) {
    if (mode == kMedian) launch_np<kBF16, kMedian>(rows, n, d, f, masks, out, out_dt, s);
    else launch_np<kBF16, kTrimmedMean>(rows, n, d, f, masks, out, out_dt, s);
  } else {
    if (mode == kMedian) launch_np<kF16, kMedian>(rows, n, d, f, masks, out, out_dt, s);
    else launch_np<kF16, kTrimmedMean>(rows, n, d, f, masks, out, out_dt, s);
  }
}

}  // namespace coord
}  // namespace gpu
}  // namespace garfield

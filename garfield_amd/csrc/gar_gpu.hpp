// Host-side launchers of the CDNA4 (gfx950) robust-aggregation kernels.
//
// Every launcher is asynchronous on the given stream, allocates nothing and
// never synchronises, so a caller may capture it into a hipGraph
// (contrast: the reference's cudaMalloc + cudaMemcpy + cudaStreamSynchronize
// inside every call, pytorch_impl/libs/native/py_krum/krum.cu:77-154).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gar_common.hpp"

namespace garfield {
namespace gpu {

// ---- Gram matrix (pairwise distances as G·Gᵀ on MFMA) ----------------------
int gram_nb(int n);                          // 16-row blocks: 1, 2, 4 or 8
int gram_padded(int n);                      // 16 * gram_nb(n)
int gram_grid(int64_t d, int dt, int n);     // split-K workgroups
int64_t gram_slab_floats(int n);             // floats per split-K slab
constexpr int kGramReduceGroups = 16;        // stage-1 partials of the slab reduction
// slabs: [grid + kGramReduceGroups][slab_floats] workspace; gram: [np][np] fp32 output
void gram(const RowTable& rows, int n, int64_t d, int dt, float* slabs, int grid,
          float* gram, hipStream_t stream);

// ---- Selection (one workgroup, on device, no host round-trip) --------------
// krum, bulyan, geomed, cclip, dnc, caf, nnm_mix and nnm_sets share gar_select.hpp: the distances from the Gram, the
// validity policy, and launch_select (1024 threads per problem, n <= kMaxRows).
// weights[n] (fp32), order[n] (gradient ids by increasing score), scores[n]
// batch > 1: `batch` independent problems, gram [batch][np][np] -> weights/order/scores [batch][n]
void krum_select(const float* gram, int np, int n, int f, int m, float* weights,
                 int* order, float* scores, hipStream_t stream, int batch = 1);

// Geometric median (gar_geomed.hip): `iters` smoothed-Weiszfeld rounds on the distances of the Gram
// (n <= kMaxRows); weights[n] = the iterate's coefficients, dists[n] = its distance r_i to every row
// (+inf on rows without a finite distance). batch as krum_select.
void geomed_select(const float* gram, int np, int n, int iters, double nu, float* weights, float* dists,
                   hipStream_t stream, int batch = 1);

// Centered clipping (gar_cclip.hip): `iters` clipping rounds on the distances of the Gram (n <= kMaxRows).
// Rows 0..nw-1 are the workers, rows nw..n-1 basis-only (an appended centre). a0[n]: the start weights
// (nullptr: uniform on the workers; may alias weights). tau > 0: the absolute L2 radius; tau <= 0: from
// the data, the max(|V| - f, 1)-th smallest distance of the centre to a valid worker, every round.
// weights[n] = the centre's coefficients, dists[n] = its distance r_i to every valid worker before the
// last round (+inf elsewhere). batch as krum_select (a0, when given, [batch][n]).
void cclip_select(const float* gram, int np, int n, int nw, const float* a0, double tau, int f, int iters,
                  float* weights, float* dists, hipStream_t stream, int batch = 1);

// DnC spectral filtering (gar_dnc.hip): `iters` power rounds on K = -½ J D J of the Gram's distances
// (n <= kMaxRows, K never stored); scores[n] = λ u_i², the squared projection of row i on the top
// principal direction (+inf on rows without a finite distance); weights[n] = 1 / kv on the
// kv = min(m, |V|) valid rows of lowest (score, index), 0 elsewhere. batch as krum_select.
void dnc_select(const float* gram, int np, int n, int m, int iters, float* weights, float* scores,
                hipStream_t stream, int batch = 1);

// CAF covariance filter (gar_caf.hip): while more than n - 2f rows' worth of weight is left (at most
// max_passes passes, 0 = n), `iters` power rounds on M = A^½ K A^½ of the Gram's distances (n <= kMaxRows,
// K never stored) and a soft down-weighting of every row by its squared projection on the top principal
// direction of the weighted covariance; weights[n] = the weights of the pass of smallest λ (0 on rows
// without a finite distance), lams[n] = λ of pass p at index p, +inf beyond the last pass. batch as krum_select.
void caf_select(const float* gram, int np, int n, int f, int iters, int max_passes, float* weights, float* lams,
                hipStream_t stream, int batch = 1);

// Nearest-neighbour mixing (gar_nnm.hip), n <= kMaxRows, 0 <= f < n, c = n - f. nnm_mix: from the Gram,
// masks[n][2] (the set S_i of row i as two 64-bit words: i and its c - 1 nearest) and the pseudo-Gram
// H [np][np] (H_ii = 0, H_ij = -D'_ij / 2 with D' the squared distances of the mixed rows), on which
// krum_select / geomed_select run unchanged. nnm_unmix: w[n] = the selection's weights a[n] over the
// mixed rows folded back onto the original rows (a and w distinct). batch as krum_select.
void nnm_mix(const float* gram, int np, int n, int f, float* H, unsigned long long* masks, hipStream_t stream,
             int batch = 1);
void nnm_unmix(const float* a, const unsigned long long* masks, int n, int f, float* w, hipStream_t stream,
               int batch = 1);

// NNM before a coordinate-wise rule (gar_nnm_coord.hip). nnm_sets: masks[n][2] alone, nnm_mix's sets bit
// for bit without its pseudo-Gram; batch as krum_select. nnm_coord: out[x] = the rule (mode kTrimmedMean
// with f, n >= 2f + 1, or kMedian) over the n mixed values (1/c) Σ_{j∈S_i} row_j[x], c = n - f, of every
// coordinate, never stored; n <= kMaxRows, dt f32 / bf16 / f16, out fp32 or the rows' dtype.
void nnm_sets(const float* gram, int np, int n, int f, unsigned long long* masks, hipStream_t stream, int batch = 1);
void nnm_coord(const RowTable& rows, int n, int64_t d, int dt, int mode, int f, const unsigned long long* masks,
               void* out, int out_dt, hipStream_t stream);

// Adaptive robust clipping (gar_arc.hip), n <= kMaxRows, 0 <= f < n, k = arc_count(n, f) = 2 f (n - f) / n.
// arc_scale: from the Gram's diagonal s, C² = the (k + 1)-th largest s by (s descending, index ascending, a
// non-finite s as +inf); scales[n] = sqrt(C² / s_i) where s_i and C² are finite and s_i > C², else 1;
// clip_rows[n + 1] = the number of rows with a scale != 1 (<= k), their indices ascending, then -1;
// gram_out [np][np] (nullptr: not written; may be gram) = (c_i c_j) G_ij, on which the selections run
// unchanged. arc_fold: w[n] = scales[n] * a[n] (w may be a). batch as krum_select.
// arc_apply: rows listed in clip_rows <- cast(scale * row) on the coordinates [lo, hi), in place; k is the
// host's bound on the count (no launch when 0); rows need no alignment; hi < 2^31.
int arc_count(int n, int f);
void arc_scale(const float* gram, int np, int n, int f, float* scales, int* clip_rows, float* gram_out,
               hipStream_t stream, int batch = 1);
void arc_fold(const float* a, const float* scales, int n, float* w, hipStream_t stream, int batch = 1);
void arc_apply(const RowTable& rows, int n, int k, int64_t lo, int64_t hi, int dt, const int* clip_rows, const float* scales,
               hipStream_t stream);

// W[t][n]: row k = uniform weights of the (m-k) best-scoring gradients at step k
// batch > 1: gram [batch][np][np] -> W [batch][t][n]
void bulyan_select(const float* gram, int np, int n, int f, int m, int t, float* W,
                   hipStream_t stream, int batch = 1);
// best: one uint64 (initialised here), weights[n]
void brute_select(const float* gram, int np, int n, int f, unsigned long long* best,
                  float* weights, hipStream_t stream);

// SMEA (gar_smea.hip): Brute's subset search with every (n - f)-subset scored by `iters` power rounds on its
// block of the Gram's distances (the top eigenvalue of the members' covariance), n <= 64 and at most 2^32
// subsets. best: one uint64 (initialised here), weights[n] = 1 / (n - f) on the winner's members, scores[0] =
// its eigenvalue. No batched form: one launch per problem.
void smea_select(const float* gram, int np, int n, int f, int iters, unsigned long long* best, float* weights,
                 float* scores, hipStream_t stream);

// ---- Weighted combine  out = Σ_j w_j g_j  (optionally fused SGD update) -----
void combine(const RowTable& rows, int n, int64_t d, int dt, const float* weights,
             void* out, int out_dt, hipStream_t stream);

struct SgdArgs {
  float lr;
  float momentum;
  float dampening;
  float weight_decay;
  int nesterov;
  int first_step;  // momentum buffer initialised to the gradient (torch.optim.SGD)
};
// shadow (optional): low-precision copy of the updated parameters (bf16/f16
// working weights of the forward/backward), written in the same pass.
void combine_sgd(const RowTable& rows, int n, int64_t d, int dt, const float* weights,
                 float* param, float* momentum_buf, float* grad_out, void* shadow, int shadow_dt,
                 SgdArgs args, hipStream_t stream);

// ---- Layer-wise GAR: the rule on every parameter segment of the flat rows ----
// jobs: [njobs][3] int64 (start, end, segment) coordinate ranges, each inside one segment, in
// segment order; seg_lo: [L + 1] int32, the first job of each segment (seg_lo[L] = njobs).
// lw_gram: gram [L][np][np] = per-segment G·Gᵀ (slabs: [njobs][gram_slab_floats(n)] workspace).
void lw_gram(const RowTable& rows, int n, int dt, const int64_t* jobs, int njobs, const int* seg_lo, int L,
             float* slabs, float* gram, hipStream_t stream);
// lw_bulyan_tail: out[x] (fp32) for every coordinate x of the jobs (LOCAL coordinates) = Bulyan's
// tail with x's segment's W[s] [t][n]: the averaged median (beta) of the t selection means
void lw_bulyan_tail(const RowTable& rows, int n, int dt, const int64_t* jobs, int njobs, const float* W, int t,
                    int beta, float* out, hipStream_t stream);
// lw_combine_sgd: per coordinate of segment s, g = Σ_j weights[s][j] row_j, then the SGD update
// of param / momentum (and the shadow copy), as combine_sgd does with one weight vector.
// jobs in LOCAL coordinates of rows / param / momentum / shadow, base = the global coordinate of
// local 0 (a sharded bucket's owned range); seg_off: [L + 1] int64 global segment offsets.
void lw_combine_sgd(const RowTable& rows, int n, int dt, const int64_t* jobs, int njobs, const float* weights,
                    float* param, float* momentum_buf, void* shadow, int shadow_dt, SgdArgs args,
                    const int64_t* seg_off, int64_t base, hipStream_t stream);

// ---- Coordinate-wise rules (median, trimmed mean, MeaMed, ...) -------------
// W/t are only read for kBulyanTail; seed/threshold only for kCondense.
void coordwise(const RowTable& rows, int n, int64_t d, int dt, int mode, int f, int beta,
               const float* W, int t, uint64_t seed, uint64_t threshold, void* out,
               int out_dt, hipStream_t stream);
int coordwise_max_rows();
// What coordwise() launches for these arguments (coord::plan of gar_coord_plan.hpp; host only, no
// GPU needed): the kernel family by name, its padded row count, grid, the coordinates one
// workgroup covers per pass of its grid-stride loop, and the family's second template choice.
struct CoordPlanInfo {
  const char* family;
  int np;
  int64_t grid;
  int64_t coords_per_pass;
  int sub;
};
CoordPlanInfo coordwise_plan(int n, int64_t d, int dt, int mode, int f, int beta, int t, bool has_W);

// ---- Large gradient sets (kMaxRows < n <= kLargeRows), one [n, ld] matrix (gar_large.hip) ----
// out[j] = Σ_i w[i] x[i, j] (out in x's dtype); mode 0 median, 1 trimmed-mean(f), 2 averaged-median(beta).
void large_combine(const void* x, int dt, int n, int64_t d, int64_t ld, const float* w, void* out, hipStream_t stream);
// fp32 Gram [n, n] of the [n, d] rows x (row stride ld) on MFMA: split-K 64 x 64 tiles into
// large_gram_slab_floats(n, d, dt) floats of slabs, then a fixed-order reduction (n <= kLargeRows)
int64_t large_gram_slab_floats(int n, int64_t d, int dt);
void large_gram(const void* x, int dt, int n, int64_t d, int64_t ld, float* slabs, float* gram, hipStream_t stream);
// V [t, d] (row stride ldv) = W [t, n] fp32 · x [n, d] (row stride ld) on fp32 MFMA
void large_wx(const float* W, int t, int n, const void* x, int dt, int64_t d, int64_t ld, float* V, int64_t ldv,
              hipStream_t stream);
// Multi-Krum (rounds 1, W [1][n] = 1/m on the m best scores) / Bulyan (rounds t, shrink: W [t][n] with
// 1/max(m - k, 1) in round k) selection from an fp32 Gram [n][ld] (n <= kLargeRows, 1 <= n - f - 2);
// thr_val / thr_idx / nearsum: [n] workspaces.
void large_select(const float* gram, int64_t ld, int n, int f, int m, int rounds, bool shrink, double* thr_val,
                  int* thr_idx, double* nearsum, float* W, hipStream_t stream);
void large_coord(const void* x, int dt, int n, int64_t d, int64_t ld, int mode, int f, int beta, void* out,
                 hipStream_t stream);

// ---- Aksel: squared distances of every gradient to a centre vector ---------
int sqdist_grid(int64_t d);
void sqdist_partial(const RowTable& rows, int n, int64_t d, int dt, const float* center,
                    float* slabs, int grid, hipStream_t stream);
// Colluding attacks (runtime/attacks.py lie / empire) in place on the exchanged rows: rows 0..P-1 the
// colluders' estimates, rows P..P+T-1 the Byzantine rows (holding their honest gradient); param = z
// (lie) or eps (empire)
void collude(const RowTable& rows, int P, int T, int64_t d, int dt, bool empire, float param, hipStream_t stream);
void aksel_select(const float* slabs, int grid, int n, int c, float* weights, float* dists,
                  hipStream_t stream);

// ---- Adaptive colluding attacks Min-Max / Min-Sum (gar_agr_attack.hip) ----------------------------
// The k <= kMaxRows rows are the colluders' estimates E: rows 0..P-1 the peers, rows P..k-1 the Byzantine
// rows (holding their honest gradient). dt f32 / bf16 / f16; rows need no alignment (16-byte loads when
// every row is 16-byte aligned at lo, single elements otherwise). Perturbation p per coordinate:
enum AgrPerturbation : int { kAgrStd = 0, kAgrUv = 1, kAgrSgn = 2 };   // -σ (unbiased), -μ, -sign μ
int agr_grid(int64_t count);   // workgroups of the streaming passes over `count` coordinates (<= 4096)
// agr_stats: partials [agr_grid(hi - lo)][k + 1] fp64, each workgroup's share of b_i = Σ_x p (μ - e_i) and
// c = Σ_x p² over the coordinates [lo, hi). agr_reduce: out[k + 1] = Σ of nparts such vectors, fixed order.
void agr_stats(const RowTable& rows, int k, int64_t lo, int64_t hi, int dt, int pert, double* partials,
               hipStream_t stream);
void agr_reduce(const double* parts, int nparts, int k, double* out, hipStream_t stream);
// agr_solve: one workgroup. parts [nparts][k + 1] summed in the same fixed order, the distances of the Gram
// [np][np] of E -> gamma[0] (fp32) and info [2 + 2k] fp64 = γ, R (Min-Max) or S (Min-Sum), a_i, b_i.
void agr_solve(const float* gram, int np, int k, const double* parts, int nparts, bool minsum, float* gamma,
               double* info, hipStream_t stream);
// agr_write: rows P..k-1 <- cast(fmaf(γ, p, μ)) on [lo, hi), γ read from device memory; nothing outside
// [lo, hi) and no row below P is written.
void agr_write(const RowTable& rows, int k, int P, int64_t lo, int64_t hi, int dt, int pert, const float* gamma,
               hipStream_t stream);

// ---- Worker-side momentum (worker_mom.hip), in place on coordinates [lo, hi) of k exchange rows ----
// X: row r at X + r * xstride elements of dtype dt (f32 / bf16 / f16); M: the fp32 state, row r at
// M + r * ld. First step: m <- g; later: m <- fmaf(beta, m, omega * g); then row <- cast(m). A
// non-finite g stays in the row and leaves m unchanged. k <= 65535, hi < 2^31.
void worker_momentum(void* X, int dt, int64_t xstride, float* M, int64_t ld, int k, int64_t lo, int64_t hi, float beta,
                     float omega, bool first, hipStream_t stream);

// ---- Split-K partial sums -> exchange rows (gar_flatten.hip) -----------------
// out[g * ostride + r * opitch + c] = Σ_s part[s * ss + g * gs + r * ipitch + c] (cast to odt),
// r < R, c < Cc, g < G.
void split_reduce(const float* part, int S, int G, int64_t R, int64_t Cc, int64_t ipitch, int64_t opitch, int64_t ss,
                  int64_t gs, void* out, int odt, int64_t ostride, hipStream_t stream);

// The same for many (part, out) pairs in one launch (up to kMaxSplitJobs per launch).
struct SplitJob {
  const float* part;
  void* out;
  int64_t R, Cc, ipitch, opitch, ss, gs, ostride;
  int S, G, odt, vec;
};
constexpr int kMaxSplitJobs = 32;   // kernarg budget: 32 x 80 B
void split_reduce_multi(const SplitJob* jobs, int count, hipStream_t stream);

// ---- Multi-tensor flatten + cast (per-parameter grads -> exchange row) -----
constexpr int kMaxFlatTensors = 96;  // tensors per launch (kernarg budget); more => several launches
int flatten_cast(const void* const* srcs, const int* src_dts, const int64_t* numels, const int64_t* offsets,
                 int count, void* dst, int out_dt, hipStream_t stream);

// ---- Stream signal: 1-thread kernel storing `value` (system-scope release) ----
void signal_set(void* p, uint64_t value, hipStream_t stream);
// host stub of the signal kernel (identifies its nodes in a captured graph)
const void* signal_kernel();
// counter signals: k_signal_add (+1, release) and a bounded device-side wait (>= target)
const void* signal_add_kernel();
void signal_add(void* p, hipStream_t stream);
void wait_geq(const void* p, uint64_t target, uint64_t timeout_us, void* err, hipStream_t stream);

}  // namespace gpu
}  // namespace garfield

// prt_energy_tolerance.hpp -- Monte Carlo tolerancing of the geometric enclosed energy from one trace, on the device
// (DESIGN.md section 4.5): the energy within given radii and the radius that holds given fractions, through focus, of
// many perturbed systems under the linear ray model.  It composes the two passes before it and adds no arithmetic of its
// own to either: the staging, the moved ray, the moments and the least-squares focus are prt_mtf_tolerance.hpp's
// (MtfgStaging, mtfg_stage, mtft_max_slices, mtft_load, mtft_move, k_mtft_moments, k_mtft_focus), the distance and the
// power-of-two integer weights are prt_energy.hpp's (energy_distance, energy_shift, energy_quantum).  include/prt.h.
//
//   k_etol_max         per (group, chunk of 1024 selected rows): the chunk's largest staged weight into the group's w_max
//                      (one integer atomic max on the double's bits per workgroup)
//   k_etol_scale       per (group, chunk): q_r = floor(ldexp(w_r, shift)), the shift from w_max and the group's count of
//                      selected rows; W = sum q (integer atomics, one per workgroup)
//   k_etol_curve<CP>   per (ray slice, trial tile, chunk of kEtolOut outputs (plane, radius), plane-major): a thread owns
//                      one trial, its coefficients, its focus shift and its centroid's four quotients in registers; the
//                      slice's rays go through the LDS tile as broadcasts; per (ray, trial) mtft_move, then per plane of
//                      the chunk one energy_distance and per output cnt += d <= R ? q : 0 in uint64 registers; partial
//                      counts into a slab (slice, trial, output)
//   k_etol_fold        per (group, trial, output): the slices added (integers: any order) into count_out; energy_out
//   k_etol_select<CP>  one pass of the most-significant-bits-first multiway bisection on the 63-bit image of d: per (ray
//                      slice, trial tile, (plane, tile of kEtolFractions fractions)), per fraction the seven counts
//                      sum q [key <= threshold_j] for the thresholds that split the prefix's interval in eight; partial
//                      counts into a slab (slice, trial, item, fraction, threshold)
//   k_etol_digit       per (group, trial, item, fraction): the slices added, the first threshold whose count reaches
//                      T = clamp(ceil(phi W), 1, W) appended to the prefix as three bits; after 21 passes the prefix is
//                      the radius
// Every sum that decides an output is an integer sum: exact in any order.  No floating-point atomics.  A group's slices
// follow its count of selected rows, n_groups and the device's CU count -- never n_rows, M, K, the output counts or the
// trial values --, and a trial's arithmetic does not depend on the other trials of the call.
#pragma once

#include <vector>

enum { ETOL_MAX_RADII = 256, ETOL_MAX_FRACTIONS = 16, ETOL_MAX_FOCUS = 256, ETOL_RECORD = 8 };
static const int kEtolOut = 8;                         // outputs of a curve chunk (uint64 counters in registers)
static const int kEtolFractions = 4;                   // fractions of a select item
static const int kEtolBits = 3;                        // bits a select pass appends to a prefix
static const int kEtolThresholds = (1 << kEtolBits) - 1;  // counters a fraction
static const int kEtolPasses = 63 / kEtolBits;         // the 63 bits of a non-negative double
static const int kEtolCell = kEtolFractions * kEtolThresholds;  // uint64 words a (slice, trial, item) of the select's slab
static const size_t kEtolSlabBytes = kMtftSlabBytes;   // cap on a launch's partial counts
static_assert(kEtolPasses * kEtolBits == 63 && kEtolCell * 8 >= MTFT_MOMENTS * 8 && kEtolCell >= kEtolOut,
              "21 passes of three bits; a trial's cell of the select holds its moments and a chunk of the curve");

// per (group, chunk of kMtfgChunk selected rows): the largest staged weight (a row left out is staged with w = 0)
__global__ void __launch_bounds__(kMtfgBlock)
k_etol_max(int n_groups, const int64_t* __restrict__ group_first, const int64_t* __restrict__ chunk_start,
           const MtfRay* __restrict__ stage, u64* __restrict__ w_max) {
  __shared__ double red[1][kMtfgBlock];
  const int t = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int g = mtf_owner(chunk_start, n_groups, chunk);
  if (g < 0) return;
  const int64_t lo = group_first[g] + (chunk - chunk_start[g]) * kMtfgChunk;
  const int64_t hi = lo + kMtfgChunk < group_first[g + 1] ? lo + kMtfgChunk : group_first[g + 1];
  double top = 0.0;
  for (int64_t r = lo + t; r < hi; r += kMtfgBlock) {
    const double w = stage[r].w;
    top = w > top ? w : top;
  }
  red[0][t] = top;
  sort_tree(red, t, [](int, double& a, double b) { a = b > a ? b : a; });
  // (weights are >= 0: the order of their bit images is their own)
  if (t == 0 && red[0][0] > 0.0) atomicMax(w_max + g, (u64)__double_as_longlong(red[0][0]));
}

// per (group, chunk): q_r = (uint64) floor(ldexp(w_r, shift)), count the group's selected rows; W[g] += the chunk's sum
__global__ void __launch_bounds__(kMtfgBlock)
k_etol_scale(int n_groups, const int64_t* __restrict__ group_first, const int64_t* __restrict__ chunk_start,
             const MtfRay* __restrict__ stage, const u64* __restrict__ w_max, u64* __restrict__ q,
             u64* __restrict__ total) {
  __shared__ u64 red[1][kMtfgBlock];
  const int t = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int g = mtf_owner(chunk_start, n_groups, chunk);
  if (g < 0) return;
  const int64_t lo = group_first[g] + (chunk - chunk_start[g]) * kMtfgChunk;
  const int64_t hi = lo + kMtfgChunk < group_first[g + 1] ? lo + kMtfgChunk : group_first[g + 1];
  const int by = energy_shift(w_max[g], (long long)(group_first[g + 1] - group_first[g]));  // (a chunk: count >= 1)
  u64 mine = 0;
  for (int64_t r = lo + t; r < hi; r += kMtfgBlock) {
    const u64 v = energy_quantum(stage[r].w, by);
    q[r] = v;
    mine += v;
  }
  red[0][t] = mine;
  sort_tree(red, t);
  if (t == 0 && red[0][0]) atomicAdd(total + g, red[0][0]);
}

// what a thread holds of its trial beside the coefficients: the focus shift and, with follow_centroid, the quotients
// m_P / m_0 and m_S / m_0 of the trial's folded moments (moments_out), each rounded on its own
struct EtolTrial { double shift, p1, p2, s1, s2; };
__device__ __forceinline__ EtolTrial etol_trial(const double* __restrict__ moments, const double* __restrict__ delta,
                                                int64_t at_moments, int64_t at_delta, bool valid, int follow) {
  EtolTrial t = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (!valid) return t;
  t.shift = delta[at_delta];
  if (follow) {
    const double* m = moments + at_moments * MTFT_MOMENTS;
    t.p1 = m[1] / m[0], t.p2 = m[2] / m[0], t.s1 = m[3] / m[0], t.s2 = m[4] / m[0];
  }
  return t;
}
// d of the moved ray in the plane at delta about the trial's centre there: c = m_P / m_0 + delta * (m_S / m_0), the
// product and the sum each rounded (no fma), or 0 about the held centre
__device__ __forceinline__ double etol_distance(const MtfRay& moved, const EtolTrial& t, double delta, int follow,
                                                int shape) {
  const double c1 = follow ? t.p1 + delta * t.s1 : 0.0, c2 = follow ? t.p2 + delta * t.s2 : 0.0;
  return energy_distance(moved, delta, c1, c2, shape);
}

// Thread t owns trial first + blockIdx.y * kMtftTile + t of the slice's group and, of it, the kEtolOut outputs of chunk
// blockIdx.z of this launch's outputs [o_first, o_first + width), output o = plane * n_radii + radius.  delta: (n_groups,
// n_trials) of this launch; moments: moments_out (n_groups, M, 8); slab: (slice, n_trials, width) counts
template <int CP>
__global__ void __launch_bounds__(kMtftBlock)
k_etol_curve(int n_groups, const int64_t* __restrict__ slice_start, const int64_t* __restrict__ group_first,
             const MtfRay* __restrict__ stage, const MtfgPar* __restrict__ stage_par, const u64* __restrict__ q,
             int64_t n_selected, int K, const double* __restrict__ trials, int M, int first, int n_trials,
             const double* __restrict__ delta, const double* __restrict__ moments, const double* __restrict__ focus,
             const double* __restrict__ radii, int n_radii, int shape, int follow, int64_t o_first, int64_t width,
             u64* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) MtfRay tile[kMtftRays];
  __shared__ __attribute__((aligned(16))) MtfgPar par[kMtftRays][CP];
  __shared__ u64 weight[kMtftRays];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int g = mtf_owner(slice_start, n_groups, s);
  if (g < 0) return;
  const int mine = (int)blockIdx.y * kMtftTile + t;  // (this thread's trial, in the launch)
  const bool busy = (int)blockIdx.y * kMtftTile + (t & ~63) < n_trials;  // (the same in a wave's lanes)
  const bool valid = mine < n_trials;
  const double* from = trials + ((int64_t)g * M + (valid ? first + mine : 0)) * K;
  const EtolTrial own = etol_trial(moments, delta, (int64_t)g * M + first + mine, (int64_t)g * n_trials + mine, valid, follow);
  double p[CP];
  u64 cnt[kEtolOut];
#pragma unroll
  for (int c = 0; c < CP; ++c) p[c] = valid && c < K ? from[c] : 0.0;
  // the chunk's outputs: the same in every lane, through uniform addresses; one past the end takes the last one's plane
  // and a radius no distance reaches, and is not stored
  const int64_t o0 = (int64_t)blockIdx.z * kEtolOut;  // (in the launch)
  // (the radii stay in scalar registers, with one bit an output that begins a plane; the planes' shifts would not fit
  // beside them and go through LDS: the first tile's barriers stand between this and their readers)
  __shared__ double shift[kEtolOut];
  double edge[kEtolOut];
  int fresh = 1, before = 0;
#pragma unroll
  for (int k = 0; k < kEtolOut; ++k) {
    const int64_t o = o_first + (o0 + k < width ? o0 + k : width - 1);
    const int plane = (int)(o / n_radii);
    if (k && plane != before) fresh |= 1 << k;
    before = plane;
    if (t == k) shift[k] = focus[plane];
    edge[k] = o0 + k < width ? radii[o - (int64_t)plane * n_radii] : -1.0;
    cnt[k] = 0;
  }
  int64_t lo, hi;
  mtf_slice(slice_start, group_first, group_first[g + 1] - group_first[g], g, s, lo, hi);
  for (int64_t base = lo; base < hi; base += kMtftRays) {
    const int count = hi - base < kMtftRays ? (int)(hi - base) : kMtftRays;
    __syncthreads();  // (the previous tile is read)
    mtft_load<CP>(stage, stage_par, n_selected, K, base, count, tile, par);
    if (t < count) weight[t] = q[base + t];
    __syncthreads();
    if (busy) {
      for (int r = 0; r < count; ++r) {
        const u64 w = weight[r];
        if (!w) continue;  // (the same in every lane: a row left out, or a weight that counts nothing)
        const MtfRay ray = tile[r];
        MtfRay moved;
        mtft_move<CP>(ray, par[r], p, moved.p1, moved.p2, moved.s1, moved.s2);
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < kEtolOut; ++k) {
          if (fresh >> k & 1) d = etol_distance(moved, own, shift[k] + own.shift, follow, shape);
          cnt[k] += d <= edge[k] ? w : 0;
        }
      }
    }
  }
  if (valid) {
    u64* o = slab + ((size_t)s * n_trials + mine) * width + o0;
#pragma unroll
    for (int k = 0; k < kEtolOut; ++k)
      if (o0 + k < width) o[k] = cnt[k];
  }
}

// per (group, trial of the launch, output of the launch): the slices' counts added; count_out and energy_out:
// (n_groups, M, n_out); a group without weight: count 0, energy NaN
__global__ void __launch_bounds__(PRT_BLOCK)
k_etol_fold(int n_groups, int64_t n_out, int64_t o_first, int64_t width, const int64_t* __restrict__ slice_start,
            const u64* __restrict__ slab, const u64* __restrict__ total, int M, int first, int n_trials,
            u64* __restrict__ count_out, double* __restrict__ energy_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * n_trials * width) return;
  const int g = (int)(item / (n_trials * width));
  const int mine = (int)((item - (int64_t)g * n_trials * width) / width);
  const int64_t o = item - ((int64_t)g * n_trials + mine) * width;
  u64 sum = 0;
  for (int64_t s = slice_start[g]; s < slice_start[g + 1]; ++s) sum += slab[((size_t)s * n_trials + mine) * width + o];
  const u64 all = total[g];
  const size_t at = ((size_t)g * M + first + mine) * n_out + o_first + o;
  count_out[at] = all ? sum : 0;
  energy_out[at] = all ? (double)sum / (double)all : __longlong_as_double(0x7ff8000000000000ll);
}

// One pass.  Thread t owns trial first + blockIdx.y * kMtftTile + t and, of it, item z_first + blockIdx.z of the
// (plane, fraction tile) items: plane = item / tiles, the fractions [tile * kEtolFractions, ...) of it.  state: (n_groups,
// n_trials, items of the launch, kEtolFractions), the prefixes found so far (`done` bits each; nothing is read at
// done = 0).  A key's place against the eight sub-intervals of a prefix is e = (key >> rest) - (prefix << 3), rest the
// bits below this pass's: key <= threshold_j exactly where e <= j.  slab: (slice, n_trials, items, kEtolFractions, 7)
template <int CP>
__global__ void __launch_bounds__(kMtftBlock)
k_etol_select(int n_groups, const int64_t* __restrict__ slice_start, const int64_t* __restrict__ group_first,
              const MtfRay* __restrict__ stage, const MtfgPar* __restrict__ stage_par, const u64* __restrict__ q,
              int64_t n_selected, int K, const double* __restrict__ trials, int M, int first, int n_trials,
              const double* __restrict__ delta, const double* __restrict__ moments, const double* __restrict__ focus,
              int n_fractions, int shape, int follow, int z_first, int items, int done, const u64* __restrict__ state,
              u64* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) MtfRay tile[kMtftRays];
  __shared__ __attribute__((aligned(16))) MtfgPar par[kMtftRays][CP];
  __shared__ u64 weight[kMtftRays];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int g = mtf_owner(slice_start, n_groups, s);
  if (g < 0) return;
  const int mine = (int)blockIdx.y * kMtftTile + t;
  const bool busy = (int)blockIdx.y * kMtftTile + (t & ~63) < n_trials;
  const bool valid = mine < n_trials;
  const double* from = trials + ((int64_t)g * M + (valid ? first + mine : 0)) * K;
  const EtolTrial own = etol_trial(moments, delta, (int64_t)g * M + first + mine, (int64_t)g * n_trials + mine, valid, follow);
  const int tiles = (n_fractions + kEtolFractions - 1) / kEtolFractions;
  const int z = z_first + (int)blockIdx.z, f = z / tiles, tile_first = (z - f * tiles) * kEtolFractions;
  const int held = n_fractions - tile_first < kEtolFractions ? n_fractions - tile_first : kEtolFractions;
  const size_t cell = ((size_t)g * n_trials + (valid ? mine : 0)) * items + blockIdx.z;
  const int rest = 63 - done - kEtolBits;
  double p[CP];
  long long low[kEtolFractions];  // (prefix << 3: where the prefix's interval begins, in units of this pass's digit)
  u64 cnt[kEtolFractions][kEtolThresholds];
#pragma unroll
  for (int c = 0; c < CP; ++c) p[c] = valid && c < K ? from[c] : 0.0;
#pragma unroll
  for (int k = 0; k < kEtolFractions; ++k) {
    low[k] = done && k < held ? (long long)(state[cell * kEtolFractions + k] << kEtolBits) : 0;
#pragma unroll
    for (int j = 0; j < kEtolThresholds; ++j) cnt[k][j] = 0;
  }
  const double plane = focus[f] + own.shift;
  int64_t lo, hi;
  mtf_slice(slice_start, group_first, group_first[g + 1] - group_first[g], g, s, lo, hi);
  for (int64_t base = lo; base < hi; base += kMtftRays) {
    const int count = hi - base < kMtftRays ? (int)(hi - base) : kMtftRays;
    __syncthreads();  // (the previous tile is read)
    mtft_load<CP>(stage, stage_par, n_selected, K, base, count, tile, par);
    if (t < count) weight[t] = q[base + t];
    __syncthreads();
    if (busy) {
      for (int r = 0; r < count; ++r) {
        const u64 w = weight[r];
        if (!w) continue;  // (the same in every lane)
        const MtfRay ray = tile[r];
        MtfRay moved;
        mtft_move<CP>(ray, par[r], p, moved.p1, moved.p2, moved.s1, moved.s2);
        const long long digit = __double_as_longlong(etol_distance(moved, own, plane, follow, shape)) >> rest;
#pragma unroll
        for (int k = 0; k < kEtolFractions; ++k) {
          const long long e = digit - low[k];
#pragma unroll
          for (int j = 0; j < kEtolThresholds; ++j) cnt[k][j] += e <= j ? w : 0;
        }
      }
    }
  }
  if (valid) {
    u64* o = slab + (((size_t)s * n_trials + mine) * items + blockIdx.z) * kEtolCell;
#pragma unroll
    for (int k = 0; k < kEtolFractions; ++k)
#pragma unroll
      for (int j = 0; j < kEtolThresholds; ++j) o[k * kEtolThresholds + j] = cnt[k][j];
  }
}

// per (group, trial of the launch, item of the launch, fraction of its tile): the slices' seven counts added; the digit
// is the first j whose count reaches T = clamp(ceil(phi W), 1, W), 7 where none does (the eighth sub-interval then holds
// it: the count up to the prefix's end reached T a pass ago); after the last pass radius_out (n_groups, M, n_focus,
// n_fractions) is the prefix; NaN at once for a group without weight
__global__ void __launch_bounds__(PRT_BLOCK)
k_etol_digit(int n_groups, const int64_t* __restrict__ slice_start, const u64* __restrict__ slab,
             const u64* __restrict__ total, const double* __restrict__ fractions, int n_fractions, int n_focus, int M,
             int first, int n_trials, int z_first, int items, int done, u64* __restrict__ state,
             double* __restrict__ radius_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * n_trials * items * kEtolFractions) return;
  const int k = (int)(item % kEtolFractions);
  const int64_t cell = item / kEtolFractions;  // (group, trial, item)
  const int zi = (int)(cell % items);
  const int mine = (int)((cell / items) % n_trials), g = (int)(cell / ((int64_t)items * n_trials));
  const int tiles = (n_fractions + kEtolFractions - 1) / kEtolFractions;
  const int z = z_first + zi, f = z / tiles, fraction = (z - f * tiles) * kEtolFractions + k;
  if (fraction >= n_fractions) return;
  double* out = radius_out + (((size_t)g * M + first + mine) * n_focus + f) * n_fractions + fraction;
  const u64 all = total[g];
  if (!all) {
    *out = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  u64 need = (u64)ceil(fractions[fraction] * (double)all);
  need = need < 1 ? 1 : (need > all ? all : need);
  u64 sum[kEtolThresholds];
#pragma unroll
  for (int j = 0; j < kEtolThresholds; ++j) sum[j] = 0;
  for (int64_t s = slice_start[g]; s < slice_start[g + 1]; ++s) {
    const u64* c = slab + (((size_t)s * n_trials + mine) * items + zi) * kEtolCell + k * kEtolThresholds;
#pragma unroll
    for (int j = 0; j < kEtolThresholds; ++j) sum[j] += c[j];
  }
  u64 digit = kEtolThresholds;
#pragma unroll
  for (int j = kEtolThresholds - 1; j >= 0; --j)
    if (sum[j] >= need) digit = (u64)j;
  const u64 prefix = ((done ? state[item] : 0) << kEtolBits) | digit;
  state[item] = prefix;
  if (done + kEtolBits == 63) *out = __longlong_as_double((long long)prefix);
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t prt_frame_energy_tolerance_workspace_bytes(int64_t n_selected, int n_groups, int n_parameters,
                                                              int n_radii, int n_fractions, int n_focus, int n_trials) {
  if (n_selected < 0 || n_groups < 1 || n_groups > 65535 || n_parameters < 1 || n_parameters > MTFG_MAX_PARAMETERS ||
      n_radii < 0 || n_radii > ETOL_MAX_RADII || n_fractions < 0 || n_fractions > ETOL_MAX_FRACTIONS ||
      n_radii + n_fractions < 1 || n_focus < 1 || n_focus > ETOL_MAX_FOCUS || n_trials < 1 || n_trials > MTFT_MAX_TRIALS)
    return PRT_ERR_ARG;
  // group, chunk and slice starts (n_groups + 1 each), centres, the staging's record, w_max, W and k_mtft_focus's record
  // a group, the radii, fractions and planes, the staged rays with their parameters and integer weights
  return (3 * ((int64_t)n_groups + 1) + 3 * (int64_t)n_groups) * 8 +
         (int64_t)n_groups * (MTFG_RECORD + 3 * n_parameters) * 8 + (2 + MTFT_RECORD) * (int64_t)n_groups * 8 +
         (int64_t)(n_radii + n_fractions + n_focus) * 8 +
         n_selected * (int64_t)(sizeof(MtfRay) + (size_t)n_parameters * sizeof(MtfgPar) + 8) + 64;
}

// record_out (n_groups, 8): the record k_mtft_focus wrote (n_groups, 7), then the group's W as its bit image (W < 2^62:
// a finite double's)
__global__ void __launch_bounds__(PRT_BLOCK)
k_etol_record(int n_groups, const double* __restrict__ focus_record, const u64* __restrict__ total,
              double* __restrict__ record_out) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  for (int k = 0; k < MTFT_RECORD; ++k) record_out[(size_t)g * ETOL_RECORD + k] = focus_record[(size_t)g * MTFT_RECORD + k];
  record_out[(size_t)g * ETOL_RECORD + MTFT_RECORD] = __longlong_as_double((long long)total[g]);
}

extern "C" int prt_frame_energy_tolerance(int device, const double* rows, int64_t ld, int64_t n_rows,
                                          const int64_t* selected, int64_t n_selected, const int64_t* group_first,
                                          int n_groups, int weight_column, const double* jacobian, const double* slopes,
                                          int n_parameters, const double* reference, const double* axes, int shape,
                                          int follow_centroid, const double* radii, int n_radii, const double* fractions,
                                          int n_fractions, const double* focus, int n_focus, const double* trials,
                                          int n_trials, int compensate_focus, uint64_t* count_out,
                                          double* energy_out, double* radius_out, double* moments_out, double* focus_out,
                                          double* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  const int K = n_parameters, M = n_trials;
  if (n_rows < 0 || ld < n_rows || n_selected < 0 || n_groups < 1 || n_groups > 65535 || !moments_out || !focus_out ||
      !record_out || !trials || !workspace || !axes || !group_first || (n_rows && !rows))
    return fail(PRT_ERR_ARG, "energy_tolerance: bad buffers");
  if (K < 1 || K > MTFG_MAX_PARAMETERS) return fail(PRT_ERR_ARG, "energy_tolerance: 1 to 16 parameters");
  if (M < 1 || M > MTFT_MAX_TRIALS) return fail(PRT_ERR_ARG, "energy_tolerance: 1 to 65536 trials");
  if (n_selected && (!selected || !jacobian || !slopes))
    return fail(PRT_ERR_ARG, "energy_tolerance: selected, jacobian and slopes where rows are selected");
  if (int bad = selection_check("energy_tolerance", n_rows, n_selected, group_first, n_groups, weight_column)) return bad;
  if (shape < PRT_ENERGY_CIRCLE || shape > PRT_ENERGY_SLIT_E2)
    return fail(PRT_ERR_ARG, "energy_tolerance: shape is PRT_ENERGY_CIRCLE, SQUARE, SLIT_E1 or SLIT_E2");
  if (n_radii < 0 || n_radii > ETOL_MAX_RADII || (n_radii && (!radii || !count_out || !energy_out)))
    return fail(PRT_ERR_ARG, "energy_tolerance: 0 to 256 radii, with count_out and energy_out");
  if (n_fractions < 0 || n_fractions > ETOL_MAX_FRACTIONS || (n_fractions && (!fractions || !radius_out)))
    return fail(PRT_ERR_ARG, "energy_tolerance: 0 to 16 fractions, with radius_out");
  if (n_radii + n_fractions < 1) return fail(PRT_ERR_ARG, "energy_tolerance: radii or fractions, not neither");
  if (!focus || n_focus < 1 || n_focus > ETOL_MAX_FOCUS)
    return fail(PRT_ERR_ARG, "energy_tolerance: 1 to 256 focus shifts");
  for (int k = 0; k < n_radii; ++k)
    if (!(radii[k] >= 0 && radii[k] < PRT_INF) || (k && !(radii[k] > radii[k - 1])))
      return fail(PRT_ERR_ARG, "energy_tolerance: radii finite, >= 0 and strictly ascending");
  for (int k = 0; k < n_fractions; ++k)
    if (!(fractions[k] > 0 && fractions[k] <= 1)) return fail(PRT_ERR_ARG, "energy_tolerance: fractions in (0, 1]");
  for (int k = 0; k < n_focus; ++k)
    if (!std::isfinite(focus[k])) return fail(PRT_ERR_ARG, "energy_tolerance: focus shifts finite");
  MtfPlan plan;  // (mtfg_stage reads its axes alone)
  int rc = mtf_axes(axes, plan.ax);
  if (rc) return rc;
  // a tile of trials must fit under the cap with a slice a group (refused before a device is touched), and then with the
  // slices the device's CU count gives: a (slice, trial) cell holds the moments, a chunk of the curve or a select item
  const std::string cap = "energy_tolerance: slices * " + std::to_string(kMtftTile) + " trials * " +
                          std::to_string(kEtolCell * 8) + " bytes above the 256 MiB slab cap";
  if ((size_t)n_groups * kMtftTile * kEtolCell * 8 > kEtolSlabBytes) return fail(PRT_ERR_ARG, cap);
  int cus = 1;
  rc = psf_device(device, &cus);
  if (rc) return rc;
  // the staging of prt_frame_mtf_tolerance: the same slices, so the same moments, focus shifts and record
  const MtfgStaging staging(group_first, n_groups, K, mtft_max_slices(cus, n_groups), workspace);
  const int64_t slice_grid = staging.slice_grid;
  // the trials of a launch, whole tiles; then the curve's outputs of a launch, whole chunks, and the select's items
  int64_t most = (int64_t)(kEtolSlabBytes / ((size_t)slice_grid * kEtolCell * 8)) / kMtftTile * kMtftTile;
  if (most < kMtftTile) return fail(PRT_ERR_ARG, cap);
  most = std::min<int64_t>(most, ((int64_t)M + kMtftTile - 1) / kMtftTile * kMtftTile);
  const int64_t n_out = (int64_t)n_focus * n_radii, all_outputs = (n_out + kEtolOut - 1) / kEtolOut * kEtolOut;
  const int64_t outputs =
      std::min<int64_t>(all_outputs, (int64_t)(kEtolSlabBytes / ((size_t)slice_grid * most * 8)) / kEtolOut * kEtolOut);
  const int n_items = n_focus * ((n_fractions + kEtolFractions - 1) / kEtolFractions);
  const int items = (int)std::min<int64_t>(
      std::min(n_items, 65535), (int64_t)(kEtolSlabBytes / ((size_t)slice_grid * most * kEtolCell * 8)));
  if (staging.chunk_grid > 0x7fffffff || slice_grid > 0x7fffffff || outputs / kEtolOut > 65535 ||
      (n_selected + kMtfgBlock - 1) / kMtfgBlock > 0x7fffffff ||
      ((int64_t)n_groups * most * std::max<int64_t>(outputs, (int64_t)items * kEtolFractions) + PRT_BLOCK - 1) / PRT_BLOCK >
          0x7fffffff)
    return fail(PRT_ERR_ARG, "energy_tolerance: too many rows or outputs for one launch");
  hipStream_t st = (hipStream_t)stream;
  // the workspace after the staging's head (prt_frame_energy_tolerance_workspace_bytes)
  const int64_t *d_group = staging.d_group, *d_chunk = staging.d_chunk, *d_slice = staging.d_slice;
  double* staged_record = staging.rest;
  u64* w_max = (u64*)(staged_record + (size_t)n_groups * (MTFG_RECORD + 3 * K));
  u64* total = w_max + n_groups;
  double* focus_record = (double*)(total + n_groups);
  double* d_radii = focus_record + (size_t)MTFT_RECORD * n_groups;
  double* d_fractions = d_radii + n_radii;
  double* planes = d_fractions + n_fractions;
  MtfRay* stage = (MtfRay*)(((uintptr_t)(planes + n_focus) + 31) & ~(uintptr_t)31);
  MtfgPar* stage_par = (MtfgPar*)(stage + n_selected);
  u64* q = (u64*)(stage_par + (size_t)K * n_selected);
  std::vector<double> host((size_t)n_radii + n_fractions + n_focus);
  for (int k = 0; k < n_radii; ++k) host[k] = radii[k];
  for (int k = 0; k < n_fractions; ++k) host[(size_t)n_radii + k] = fractions[k];
  for (int k = 0; k < n_focus; ++k) host[(size_t)n_radii + n_fractions + k] = focus[k];
  const int64_t held = std::min<int64_t>(most, M);  // (trials of the largest launch)
  const size_t centre_bytes = staging.centre_bytes, delta_bytes = (size_t)n_groups * held * sizeof(double);
  const size_t state_bytes = (size_t)n_groups * held * std::max(items, 1) * kEtolFractions * sizeof(u64);
  // (one slab, for the moments, then a launch of the curve, then a launch of the select: each is folded before the next)
  const size_t cell_words = std::max<size_t>(std::max<size_t>(MTFT_MOMENTS, std::min<int64_t>(outputs, n_out)),
                                             n_fractions ? (size_t)items * kEtolCell : 0);
  const size_t slab_bytes = (size_t)slice_grid * held * cell_words * 8;
  char* scratch = nullptr;
  HIP_TRY(hipMallocAsync((void**)&scratch, centre_bytes + delta_bytes + state_bytes + slab_bytes, st));
  double* delta = (double*)(scratch + centre_bytes);
  u64* state = (u64*)(scratch + centre_bytes + delta_bytes);
  char* slab = scratch + centre_bytes + delta_bytes + state_bytes;
  HIP_TRY(hipMemsetAsync(w_max, 0, 2 * (size_t)n_groups * sizeof(u64), st));
  HIP_TRY(hipMemcpyAsync(d_radii, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, st));
  rc = mtfg_stage(staging, rows, ld, n_rows, selected, n_selected, n_groups, weight_column, jacobian, slopes, K, reference,
                  plan, (double*)scratch, staged_record, stage, stage_par, st);
  if (rc) return rc;
  if (staging.chunk_grid) {
    hipLaunchKernelGGL(k_etol_max, dim3((unsigned)staging.chunk_grid), dim3(kMtfgBlock), 0, st, n_groups, d_group, d_chunk,
                       stage, w_max);
    hipLaunchKernelGGL(k_etol_scale, dim3((unsigned)staging.chunk_grid), dim3(kMtfgBlock), 0, st, n_groups, d_group,
                       d_chunk, stage, w_max, q, total);
  }
  const int follow = follow_centroid ? 1 : 0;
  // the smallest instantiation that holds the parameters; the trials in launches of at most `most`, and under each the
  // curve's outputs in launches of at most `outputs` and the select's items in launches of at most `items`
  auto launch = [&](auto held_columns, int first, int n) {
    constexpr int CP = decltype(held_columns)::value;
    const unsigned tiles = (unsigned)((n + kMtftTile - 1) / kMtftTile);
    hipLaunchKernelGGL(k_mtft_moments<CP>, dim3((unsigned)slice_grid, tiles), dim3(kMtftBlock), 0, st, n_groups, d_slice,
                       d_group, stage, stage_par, n_selected, K, trials, M, first, n, (double*)slab);
    hipLaunchKernelGGL(k_mtft_focus, dim3((unsigned)(((int64_t)n_groups * n + PRT_BLOCK - 1) / PRT_BLOCK)),
                       dim3(PRT_BLOCK), 0, st, n_groups, K, d_slice, (const double*)slab, M, first, n,
                       compensate_focus ? 1 : 0, staged_record, moments_out, focus_out, delta, focus_record);
    for (int64_t o_first = 0; o_first < n_out; o_first += outputs) {
      const int64_t width = std::min<int64_t>(outputs, n_out - o_first);
      hipLaunchKernelGGL(k_etol_curve<CP>, dim3((unsigned)slice_grid, tiles, (unsigned)((width + kEtolOut - 1) / kEtolOut)),
                         dim3(kMtftBlock), 0, st, n_groups, d_slice, d_group, stage, stage_par, q, n_selected, K, trials, M,
                         first, n, delta, moments_out, planes, d_radii, n_radii, shape, follow, o_first, width, (u64*)slab);
      hipLaunchKernelGGL(k_etol_fold, dim3((unsigned)(((int64_t)n_groups * n * width + PRT_BLOCK - 1) / PRT_BLOCK)),
                         dim3(PRT_BLOCK), 0, st, n_groups, n_out, o_first, width, d_slice, (const u64*)slab, total, M, first,
                         n, (u64*)count_out, energy_out);
    }
    for (int z_first = 0; n_fractions && z_first < n_items; z_first += items) {
      const int now = std::min(items, n_items - z_first);
      for (int done = 0; done < 63; done += kEtolBits) {
        hipLaunchKernelGGL(k_etol_select<CP>, dim3((unsigned)slice_grid, tiles, (unsigned)now), dim3(kMtftBlock), 0, st,
                           n_groups, d_slice, d_group, stage, stage_par, q, n_selected, K, trials, M, first, n, delta,
                           moments_out, planes, n_fractions, shape, follow, z_first, now, done, state, (u64*)slab);
        hipLaunchKernelGGL(k_etol_digit,
                           dim3((unsigned)(((int64_t)n_groups * n * now * kEtolFractions + PRT_BLOCK - 1) / PRT_BLOCK)),
                           dim3(PRT_BLOCK), 0, st, n_groups, d_slice, (const u64*)slab, total, d_fractions, n_fractions,
                           n_focus, M, first, n, z_first, now, done, state, radius_out);
      }
    }
  };
  trial_launches(M, most, [&](int first, int n) { trial_columns<MTFG_MAX_PARAMETERS>(K, launch, first, n); });
  // (the record's first seven doubles are k_mtft_focus's; the eighth is this pass's)
  hipLaunchKernelGGL(k_etol_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     n_groups, focus_record, total, record_out);
  return mtf_finish(st, scratch);  // (it drains the stream: the host starts and tables outlive their copies, too)
}

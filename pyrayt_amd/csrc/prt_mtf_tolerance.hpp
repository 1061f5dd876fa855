// prt_mtf_tolerance.hpp -- Monte Carlo tolerancing of the geometric MTF from one trace, on the device (DESIGN.md section
// 4.5): the OTF through focus, the second moments of the landing points and the least-squares focus of many perturbed
// systems under the linear ray model, P = p + sum_k t_k dp_k and S = s + sum_k t_k ds_k the landing point and the slope
// of a ray in a trial, the merit itself not linearised.  It stands on the staging of the MTF sensitivities
// (prt_mtf_gradient.hpp: MtfgStaging and mtfg_stage, with this pass's own slice limit), on the MTF's core (prt_mtf.hpp:
// mtf_plan, mtf_slices, mtf_slice, mtf_phasor, mtf_finish), on prt_selection.hpp and on prt_trials.hpp.  include/prt.h.
//
//   k_mtft_moments<CP>  per (ray slice of a group, trial tile): a thread owns one trial, its CP >= K coefficients in
//                       registers (the rest zeros); the slice's rays go through an LDS tile (MtfRay + CP MtfgPar a ray)
//                       and are read as broadcasts; per (ray, trial) 4 CP multiply-adds for P and S, then sum w and the
//                       seven weighted sums; partial sums into a slab (slice, trial, 8)
//   k_mtft_focus        per (group, trial): the slices added in slice order into moments_out, and the trial's focus
//                       shift (the least-squares one, or 0); the first trial of a call also writes the group's record
//   k_mtft_sum<CP>      per (ray slice, trial tile, chunk of kMtftOut outputs): P and S as above, the ray moved to the
//                       trial's plane, fma(delta_m, S, P), then per output of the chunk mtf_phasor and two multiply-adds
//                       into fp64 accumulators in registers; the chunk's (kc, ks, kc delta_f, ks delta_f) is the same in
//                       every lane and is read through uniform addresses; partial sums into a slab (slice, trial, output)
//   k_mtft_fold         per (group, trial, output): the slices added in slice order, normalised by sum w in that order
// A group's slices follow its count of selected rows, n_groups and the device's CU count -- never n_rows, the frame's
// other rows, M, K, the output count or the trial values --, and a trial's arithmetic does not depend on the other trials
// of the call.  No floating-point atomics: every output is the same, bit for bit, on every run.
#pragma once

#include <vector>

enum { MTFT_MAX_TRIALS = 65536, MTFT_RECORD = 7, MTFT_MOMENTS = 8 };
static const int kMtftBlock = 256;                  // threads of a moments / sum workgroup
static const int kMtftTrials = 1;                   // trials a thread owns (coefficients and accumulators in registers)
static const int kMtftTile = kMtftBlock * kMtftTrials;  // trials of a workgroup
static const int kMtftOut = 8;                      // outputs of a chunk (fp64 complex accumulators in registers)
static const int kMtftRays = 64;                    // rays of the LDS tile
static const int kMtftColumnStep = 4;               // k_mtft_sum and k_mtft_moments are built for 4, 8, 12 and 16 columns
static const int kMtftSlicesPerCu = 4;              // slices of all groups together: about this many a CU
static const size_t kMtftSlabBytes = kMtfSlabBytes; // cap on a launch's partial sums (moments and outputs together)
static_assert(kMtftTrials == 1, "k_mtft_moments and k_mtft_sum: a trial a thread");

// the slices a group may have at most: n_groups and the CU count decide it
static int64_t mtft_max_slices(int cus, int n_groups) {
  const int64_t s = ((int64_t)kMtftSlicesPerCu * cus + n_groups - 1) / n_groups;
  return s < 1 ? 1 : (s > kMtfMaxSlices ? kMtfMaxSlices : s);
}

// the ray tile of a slice, rays [base, base + count): tile[r] the ray, par[r][j] its parameter j (zeros from K on)
template <int CP>
__device__ __forceinline__ void mtft_load(const MtfRay* __restrict__ stage, const MtfgPar* __restrict__ stage_par,
                                          int64_t n_selected, int K, int64_t base, int count, MtfRay* tile,
                                          MtfgPar (*par)[CP]) {
  const int t = threadIdx.x;
  if (t < count) tile[t] = stage[base + t];
  for (int item = t; item < CP * kMtftRays; item += kMtftBlock) {
    const int j = item / kMtftRays, r = item - j * kMtftRays;  // (a wave reads 64 rays of one parameter)
    if (r < count) par[r][j] = j < K ? stage_par[(int64_t)j * n_selected + base + r] : MtfgPar{0.0, 0.0, 0.0, 0.0};
  }
}

// the ray in a trial: P = p + sum t_k dp_k, S = s + sum t_k ds_k, the parameters in their order, each term an fma
template <int CP>
__device__ __forceinline__ void mtft_move(const MtfRay& ray, const MtfgPar* __restrict__ d, const double (&p)[CP],
                                          double& p1, double& p2, double& s1, double& s2) {
  p1 = ray.p1, p2 = ray.p2, s1 = ray.s1, s2 = ray.s2;
#pragma unroll
  for (int k = 0; k < CP; ++k) {
    const MtfgPar q = d[k];
    p1 = fma(p[k], q.dp1, p1);
    p2 = fma(p[k], q.dp2, p2);
    s1 = fma(p[k], q.ds1, s1);
    s2 = fma(p[k], q.ds2, s2);
  }
}

// Thread t owns trial first + blockIdx.y * kMtftTile + t of the slice's group.  trials: (n_groups, M, K); slab: (slice,
// n_trials, 8) of this launch's trials: sum w, sum w P (2), sum w S (2), sum w P.P, sum w P.S, sum w S.S
template <int CP>
__global__ void __launch_bounds__(kMtftBlock)
k_mtft_moments(int n_groups, const int64_t* __restrict__ slice_start, const int64_t* __restrict__ group_first,
               const MtfRay* __restrict__ stage, const MtfgPar* __restrict__ stage_par, int64_t n_selected, int K,
               const double* __restrict__ trials, int M, int first, int n_trials, double* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) MtfRay tile[kMtftRays];
  __shared__ __attribute__((aligned(16))) MtfgPar par[kMtftRays][CP];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int g = mtf_owner(slice_start, n_groups, s);
  if (g < 0) return;
  const int mine = (int)blockIdx.y * kMtftTile + t;  // (this thread's trial, in the launch)
  const bool busy = (int)blockIdx.y * kMtftTile + (t & ~63) < n_trials;  // (the same in a wave's lanes)
  const bool valid = mine < n_trials;
  const double* from = trials + ((int64_t)g * M + (valid ? first + mine : 0)) * K;
  double p[CP], m[MTFT_MOMENTS];
#pragma unroll
  for (int c = 0; c < CP; ++c) p[c] = valid && c < K ? from[c] : 0.0;
#pragma unroll
  for (int q = 0; q < MTFT_MOMENTS; ++q) m[q] = 0.0;
  int64_t lo, hi;
  mtf_slice(slice_start, group_first, group_first[g + 1] - group_first[g], g, s, lo, hi);
  for (int64_t base = lo; base < hi; base += kMtftRays) {
    const int count = hi - base < kMtftRays ? (int)(hi - base) : kMtftRays;
    __syncthreads();  // (the previous tile is read)
    mtft_load<CP>(stage, stage_par, n_selected, K, base, count, tile, par);
    __syncthreads();
    if (busy) {
      for (int r = 0; r < count; ++r) {
        const MtfRay ray = tile[r];
        double p1, p2, s1, s2;
        mtft_move<CP>(ray, par[r], p, p1, p2, s1, s2);
        const double wp1 = ray.w * p1, wp2 = ray.w * p2, ws1 = ray.w * s1, ws2 = ray.w * s2;
        m[0] += ray.w;
        m[1] += wp1;
        m[2] += wp2;
        m[3] += ws1;
        m[4] += ws2;
        m[5] = fma(wp1, p1, fma(wp2, p2, m[5]));
        m[6] = fma(wp1, s1, fma(wp2, s2, m[6]));
        m[7] = fma(ws1, s1, fma(ws2, s2, m[7]));
      }
    }
  }
  if (valid) {
    double* o = slab + ((size_t)s * n_trials + mine) * MTFT_MOMENTS;
#pragma unroll
    for (int q = 0; q < MTFT_MOMENTS; ++q) o[q] = m[q];
  }
}

// per (group, trial of the launch): the slices in slice order into moments_out (n_groups, M, 8); the focus shift of the
// trial into delta (n_groups, n_trials) and focus_out (n_groups, M): -cov(P, S) / var(S) where compensate and var(S) > 0,
// else 0; NaN for a group without weight.  Trial 0 of the call: record_out (n_groups, 7) from the staging's record
// (n_groups, 7 + 3 K): C_g, sum w in slice order, rays kept, missed, unfollowed
__global__ void __launch_bounds__(PRT_BLOCK)
k_mtft_focus(int n_groups, int K, const int64_t* __restrict__ slice_start, const double* __restrict__ slab, int M,
             int first, int n_trials, int compensate, const double* __restrict__ staged_record,
             double* __restrict__ moments_out, double* __restrict__ focus_out, double* __restrict__ delta,
             double* __restrict__ record_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * n_trials) return;
  const int g = (int)(item / n_trials), mine = (int)(item - (int64_t)g * n_trials);
  double m[MTFT_MOMENTS];
#pragma unroll
  for (int q = 0; q < MTFT_MOMENTS; ++q) m[q] = 0.0;
  for (int64_t s = slice_start[g]; s < slice_start[g + 1]; ++s) {
    const double* p = slab + ((size_t)s * n_trials + mine) * MTFT_MOMENTS;
#pragma unroll
    for (int q = 0; q < MTFT_MOMENTS; ++q) m[q] += p[q];
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool lit = m[0] > 0.0;  // (a group without kept rays, or without weight: NaN)
  double* o = moments_out + ((size_t)g * M + first + mine) * MTFT_MOMENTS;
#pragma unroll
  for (int q = 0; q < MTFT_MOMENTS; ++q) o[q] = lit ? m[q] : nan;
  double shift = lit ? 0.0 : nan;
  if (lit && compensate) {
    const double p1 = m[1] / m[0], p2 = m[2] / m[0], s1 = m[3] / m[0], s2 = m[4] / m[0];
    const double cov = m[6] / m[0] - fma(p1, s1, p2 * s2), var = m[7] / m[0] - fma(s1, s1, s2 * s2);
    if (var > 0.0) shift = -cov / var;
  }
  focus_out[(size_t)g * M + first + mine] = shift;
  delta[item] = shift;
  if (first + mine == 0) {
    const double* from = staged_record + (size_t)g * (MTFG_RECORD + 3 * K);
    double* r = record_out + (size_t)g * MTFT_RECORD;
    for (int k = 0; k < MTFT_RECORD; ++k) r[k] = from[k];
    r[3] = m[0];
  }
}

// Thread t owns trial first + blockIdx.y * kMtftTile + t of the slice's group and, of it, the kMtftOut outputs of chunk
// blockIdx.z of this launch's outputs [o_first, o_first + width).  table: (kc, ks, kc delta_f, ks delta_f) per output
// (plane, azimuth, frequency); delta: (n_groups, n_trials) of this launch; slab: (slice, n_trials, width, 2), the sums of
// w (cos, sin)
template <int CP>
__global__ void __launch_bounds__(kMtftBlock)
k_mtft_sum(int n_groups, const int64_t* __restrict__ slice_start, const int64_t* __restrict__ group_first,
           const MtfRay* __restrict__ stage, const MtfgPar* __restrict__ stage_par, int64_t n_selected, int K,
           const double* __restrict__ trials, int M, int first, int n_trials, const double* __restrict__ delta,
           const double* __restrict__ table, int64_t o_first, int64_t width, double* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) MtfRay tile[kMtftRays];
  __shared__ __attribute__((aligned(16))) MtfgPar par[kMtftRays][CP];
  __shared__ __attribute__((aligned(16))) double plane[kMtftOut][2];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int g = mtf_owner(slice_start, n_groups, s);
  if (g < 0) return;
  const int mine = (int)blockIdx.y * kMtftTile + t;  // (this thread's trial, in the launch)
  const bool busy = (int)blockIdx.y * kMtftTile + (t & ~63) < n_trials;  // (the same in a wave's lanes)
  const bool valid = mine < n_trials;
  const double* from = trials + ((int64_t)g * M + (valid ? first + mine : 0)) * K;
  const double shift = valid ? delta[(int64_t)g * n_trials + mine] : 0.0;
  double p[CP], re[kMtftOut], im[kMtftOut];
#pragma unroll
  for (int c = 0; c < CP; ++c) p[c] = valid && c < K ? from[c] : 0.0;
  // the chunk's outputs: the same addresses in every lane (one past the end reads output 0 and is not stored)
  const int64_t o0 = (int64_t)blockIdx.z * kMtftOut;  // (in the launch)
  // (kc, ks) stay in scalar registers; (kc delta_f, ks delta_f) would not fit beside them and go through LDS
  double kc[kMtftOut], ks[kMtftOut];
#pragma unroll
  for (int q = 0; q < kMtftOut; ++q) {
    const double* row = table + 4 * (o_first + (o0 + q < width ? o0 + q : 0));
    kc[q] = row[0], ks[q] = row[1];
    re[q] = im[q] = 0.0;
  }
  if (t < kMtftOut) {  // (the first tile's barriers stand between this and its readers)
    const double* row = table + 4 * (o_first + (o0 + t < width ? o0 + t : 0));
    plane[t][0] = row[2], plane[t][1] = row[3];
  }
  int64_t lo, hi;
  mtf_slice(slice_start, group_first, group_first[g + 1] - group_first[g], g, s, lo, hi);
  for (int64_t base = lo; base < hi; base += kMtftRays) {
    const int count = hi - base < kMtftRays ? (int)(hi - base) : kMtftRays;
    __syncthreads();  // (the previous tile is read)
    mtft_load<CP>(stage, stage_par, n_selected, K, base, count, tile, par);
    __syncthreads();
    if (busy) {
      for (int r = 0; r < count; ++r) {
        const MtfRay ray = tile[r];
        MtfRay moved;
        double p1, p2;
        mtft_move<CP>(ray, par[r], p, p1, p2, moved.s1, moved.s2);
        moved.p1 = fma(shift, moved.s1, p1);
        moved.p2 = fma(shift, moved.s2, p2);
        moved.w = ray.w;
        int here = 0;  // (opaque, so that the planes' products are read per ray and do not settle in 32 more registers)
        asm volatile("" : "+v"(here));
#pragma unroll
        for (int q = 0; q < kMtftOut; ++q) {
          // the phasor with the first-order correction for what the conversion to fp32 drops, as k_mtfg_sum folds it in
          double c, sn;
          const double theta = mtf_phasor(kc[q], ks[q], plane[here + q][0], plane[here + q][1], moved, c, sn);
          re[q] = fma(ray.w, fma(-theta, sn, c), re[q]);
          im[q] = fma(ray.w, fma(theta, c, sn), im[q]);
        }
      }
    }
  }
  if (valid) {
    double* o = slab + (((size_t)s * n_trials + mine) * width + o0) * 2;
#pragma unroll
    for (int q = 0; q < kMtftOut; ++q)
      if (o0 + q < width) {
        o[2 * q] = re[q];
        o[2 * q + 1] = im[q];
      }
  }
}

// per (group, trial of the launch, output of the launch): the slices in slice order; OTF = (sum w cos, -sum w sin) /
// sum w, sum w the moments' own (slab of k_mtft_moments), added in the same order; otf_out: (n_groups, M, n_out, 2)
__global__ void __launch_bounds__(PRT_BLOCK)
k_mtft_fold(int n_groups, int64_t n_out, int64_t o_first, int64_t width, const int64_t* __restrict__ slice_start,
            const double* __restrict__ slab, const double* __restrict__ moment_slab, int M, int first, int n_trials,
            double* __restrict__ otf_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * n_trials * width) return;
  const int g = (int)(item / (n_trials * width));
  const int mine = (int)((item - (int64_t)g * n_trials * width) / width);
  const int64_t o = item - ((int64_t)g * n_trials + mine) * width;
  double re = 0.0, im = 0.0, sw = 0.0;
  for (int64_t s = slice_start[g]; s < slice_start[g + 1]; ++s) {
    const double* p = slab + (((size_t)s * n_trials + mine) * width + o) * 2;
    re += p[0];
    im += p[1];
    sw += moment_slab[((size_t)s * n_trials + mine) * MTFT_MOMENTS];
  }
  double* out = otf_out + (((size_t)g * M + first + mine) * n_out + o_first + o) * 2;
  out[0] = re / sw;  // (a group without rays, or with sum w = 0: 0 / 0, NaN)
  out[1] = -im / sw;
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t prt_frame_mtf_tolerance_workspace_bytes(int64_t n_selected, int n_groups, int n_parameters,
                                                           int n_frequencies, int n_azimuths, int n_focus, int n_trials) {
  if (n_selected < 0 || n_groups < 1 || n_groups > 65535 || n_parameters < 1 || n_parameters > MTFG_MAX_PARAMETERS ||
      n_frequencies < 1 || n_frequencies > MTF_MAX_FREQUENCIES || n_azimuths < 1 || n_azimuths > MTF_MAX_AZIMUTHS ||
      n_focus < 1 || n_focus > MTF_MAX_FOCUS || n_trials < 1 || n_trials > MTFT_MAX_TRIALS)
    return PRT_ERR_ARG;
  // group, chunk and slice starts (n_groups + 1 each), centres, the staging's record, the outputs' table, the staged rays
  return (3 * ((int64_t)n_groups + 1) + 3 * (int64_t)n_groups) * 8 +
         (int64_t)n_groups * (MTFG_RECORD + 3 * n_parameters) * 8 +
         (int64_t)n_focus * n_azimuths * n_frequencies * 4 * 8 +
         n_selected * (int64_t)(sizeof(MtfRay) + (size_t)n_parameters * sizeof(MtfgPar)) + 64;
}

extern "C" int prt_frame_mtf_tolerance(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                                       int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                                       const double* jacobian, const double* slopes, int n_parameters,
                                       const double* reference, const double* axes, const double* frequencies,
                                       int n_frequencies, const double* azimuths_deg, int n_azimuths, const double* focus,
                                       int n_focus, const double* trials, int n_trials, int compensate_focus,
                                       double* otf_out, double* moments_out, double* focus_out, double* record_out,
                                       void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  const int K = n_parameters, M = n_trials;
  if (n_rows < 0 || ld < n_rows || n_selected < 0 || n_groups < 1 || n_groups > 65535 || !otf_out || !moments_out ||
      !focus_out || !record_out || !trials || !workspace || !axes || !group_first || (n_rows && !rows))
    return fail(PRT_ERR_ARG, "mtf_tolerance: bad buffers");
  if (K < 1 || K > MTFG_MAX_PARAMETERS) return fail(PRT_ERR_ARG, "mtf_tolerance: 1 to 16 parameters");
  if (M < 1 || M > MTFT_MAX_TRIALS) return fail(PRT_ERR_ARG, "mtf_tolerance: 1 to 65536 trials");
  if (n_selected && (!selected || !jacobian || !slopes))
    return fail(PRT_ERR_ARG, "mtf_tolerance: selected, jacobian and slopes where rows are selected");
  if (int bad = selection_check("mtf_tolerance", n_rows, n_selected, group_first, n_groups, weight_column)) return bad;
  // the core's checks of the sampling, its axes and its (kc, ks) table; the slices and the tiles are this pass's own
  MtfPlan plan;
  int rc = mtf_plan("mtf_tolerance", frequencies, n_frequencies, azimuths_deg, n_azimuths, focus, n_focus, axes, n_groups,
                    16, kMtftOut, kMtftBlock, plan);
  if (rc) return rc;
  const int n_k = plan.n_k;
  const int64_t n_out = plan.n_out, all_outputs = (n_out + kMtftOut - 1) / kMtftOut * kMtftOut;
  // (kc, ks, kc delta_f, ks delta_f) per output, the products as k_mtf_sum forms them
  std::vector<double> table(4 * (size_t)n_out);
  for (int64_t o = 0; o < n_out; ++o) {
    const int64_t f = o / n_k, k = o - f * n_k;
    const double kc = plan.host[2 * k], ks = plan.host[2 * k + 1], shift = plan.host[2 * (size_t)n_k + f];
    table[4 * o] = kc, table[4 * o + 1] = ks, table[4 * o + 2] = kc * shift, table[4 * o + 3] = ks * shift;
  }
  // a tile of trials and a chunk of outputs must fit under the cap with a slice a group (refused before a device is
  // touched), and then with the slices the device's CU count gives
  const std::string cap = "mtf_tolerance: slices * " + std::to_string(kMtftTile) + " trials * (" +
                          std::to_string(kMtftOut) + " outputs * 16 + 64) bytes above the 256 MiB slab cap";
  if ((size_t)n_groups * kMtftTile * (MTFT_MOMENTS * 8 + (size_t)kMtftOut * 16) > kMtftSlabBytes) return fail(PRT_ERR_ARG, cap);
  int cus = 1;
  rc = psf_device(device, &cus);
  if (rc) return rc;
  // the staging of prt_frame_mtf_gradient, the slices cut by this pass's own limit
  const MtfgStaging staging(group_first, n_groups, K, mtft_max_slices(cus, n_groups), workspace);
  const int64_t slice_grid = staging.slice_grid;
  // a launch's partial sums (the moments, and the outputs of the launch) stay under the cap: first the outputs of a
  // launch, whole chunks, as many as one tile of trials leaves room for; then the trials of a launch, whole tiles
  const int64_t tile_room = (int64_t)(kMtftSlabBytes / ((size_t)slice_grid * kMtftTile)) - MTFT_MOMENTS * 8;
  const int64_t outputs = std::min<int64_t>(all_outputs, tile_room / 16 / kMtftOut * kMtftOut);
  if (outputs < kMtftOut) return fail(PRT_ERR_ARG, cap);
  const size_t trial_bytes = (size_t)slice_grid * (MTFT_MOMENTS * 8 + (size_t)outputs * 16);
  int64_t most = (int64_t)(kMtftSlabBytes / trial_bytes) / kMtftTile * kMtftTile;
  most = std::min<int64_t>(most, ((int64_t)M + kMtftTile - 1) / kMtftTile * kMtftTile);
  if (staging.chunk_grid > 0x7fffffff || slice_grid > 0x7fffffff || outputs / kMtftOut > 65535 ||
      (n_selected + kMtfgBlock - 1) / kMtfgBlock > 0x7fffffff ||
      ((int64_t)n_groups * most * outputs + PRT_BLOCK - 1) / PRT_BLOCK > 0x7fffffff)
    return fail(PRT_ERR_ARG, "mtf_tolerance: too many rows or outputs for one launch");
  hipStream_t st = (hipStream_t)stream;
  // the workspace after the staging's head (prt_frame_mtf_tolerance_workspace_bytes)
  const int64_t *d_group = staging.d_group, *d_slice = staging.d_slice;
  double* staged_record = staging.rest;
  double* d_table = staged_record + (size_t)n_groups * (MTFG_RECORD + 3 * K);
  MtfRay* stage = (MtfRay*)(((uintptr_t)(d_table + 4 * (size_t)n_out) + 31) & ~(uintptr_t)31);
  MtfgPar* stage_par = (MtfgPar*)(stage + n_selected);
  const int64_t held = std::min<int64_t>(most, M);  // (trials of the largest launch)
  const size_t centre_bytes = staging.centre_bytes, delta_bytes = (size_t)n_groups * held * sizeof(double);
  const size_t moment_bytes = (size_t)slice_grid * held * MTFT_MOMENTS * sizeof(double);
  const size_t slab_bytes = (size_t)slice_grid * held * std::min<int64_t>(outputs, n_out) * 2 * sizeof(double);
  char* scratch = nullptr;
  HIP_TRY(hipMallocAsync((void**)&scratch, centre_bytes + delta_bytes + moment_bytes + slab_bytes, st));
  double* delta = (double*)(scratch + centre_bytes);
  double* moment_slab = (double*)(scratch + centre_bytes + delta_bytes);
  double* slab = (double*)(scratch + centre_bytes + delta_bytes + moment_bytes);
  HIP_TRY(hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, st));
  rc = mtfg_stage(staging, rows, ld, n_rows, selected, n_selected, n_groups, weight_column, jacobian, slopes, K, reference,
                  plan, (double*)scratch, staged_record, stage, stage_par, st);
  if (rc) return rc;
  // the smallest instantiation that holds the parameters; the trials in launches of at most `most`, and under each the
  // outputs in launches of at most `outputs`
  auto launch = [&](auto held_columns, int first, int n) {
    constexpr int CP = decltype(held_columns)::value;
    const unsigned tiles = (unsigned)((n + kMtftTile - 1) / kMtftTile);
    hipLaunchKernelGGL(k_mtft_moments<CP>, dim3((unsigned)slice_grid, tiles), dim3(kMtftBlock), 0, st, n_groups, d_slice,
                       d_group, stage, stage_par, n_selected, K, trials, M, first, n, moment_slab);
    hipLaunchKernelGGL(k_mtft_focus, dim3((unsigned)(((int64_t)n_groups * n + PRT_BLOCK - 1) / PRT_BLOCK)),
                       dim3(PRT_BLOCK), 0, st, n_groups, K, d_slice, moment_slab, M, first, n, compensate_focus ? 1 : 0,
                       staged_record, moments_out, focus_out, delta, record_out);
    for (int64_t o_first = 0; o_first < n_out; o_first += outputs) {
      const int64_t width = std::min<int64_t>(outputs, n_out - o_first);
      hipLaunchKernelGGL(k_mtft_sum<CP>, dim3((unsigned)slice_grid, tiles, (unsigned)((width + kMtftOut - 1) / kMtftOut)),
                         dim3(kMtftBlock), 0, st, n_groups, d_slice, d_group, stage, stage_par, n_selected, K, trials, M,
                         first, n, delta, d_table, o_first, width, slab);
      hipLaunchKernelGGL(k_mtft_fold, dim3((unsigned)(((int64_t)n_groups * n * width + PRT_BLOCK - 1) / PRT_BLOCK)),
                         dim3(PRT_BLOCK), 0, st, n_groups, n_out, o_first, width, d_slice, slab, moment_slab, M, first, n,
                         otf_out);
    }
  };
  trial_launches(M, most, [&](int first, int n) { trial_columns<MTFG_MAX_PARAMETERS>(K, launch, first, n); });
  return mtf_finish(st, scratch);  // (it drains the stream: the host starts and table outlive their copies, too)
}

// prt_mtf_gradient.hpp -- d(OTF)/d(parameter) of the geometric MTF through focus, on the device,
// from the rows, the Jacobian and the slopes a sensitivity pass left there.  Definitions: include/prt.h.
//
//   k_mtfg_centre   per (group, chunk of 1024 selected rows): rays kept / missed / unfollowed, sum w, sum w Q and
//                   sum w dQ_k, each in a fixed tree
//   k_mtfg_centre_fold  per (group, quantity): the chunks' sums added in a fixed order
//   k_mtfg_record   per group: the centre (the centroid or the given reference), the counts and dC_k
//   k_mtfg_stage    per selected row: (p1, p2, s1, s2, w) about the group's centre and, per parameter,
//                   (dp1, dp2, ds1, ds2); a row that is left out is staged with w = 0 and zeros
//   k_mtfg_sum<P>   per (ray slice of a group, output tile, chunk of P parameters): the phasor once per (ray, output),
//                   then P times four multiply-adds for g = k.dx_k and two to accumulate g w (sin, cos); the ray tile is
//                   read through LDS; partial sums go into a slab of their own
//   k_mtfg_fold     per (group, quantity, output): the slices added in slice order, normalised by sum w in that order
// The selection arrives ordered by group (group_first), so there is no sort: a row that is left out keeps its place with
// w = 0.  Every partition of the rays (chunks, slices, tiles) depends only on the group's count of selected rows, on the
// output count and on n_groups, never on the frame's other rows and never on K; a parameter's arithmetic does not depend
// on its place in the call.  No floating-point atomics: every output is the same, bit for bit, on every run.
// The staging (MtfgStaging, mtfg_stage) serves prt_frame_mtf_tolerance too; the selection's checks are prt_selection.hpp's.
// The checks and the plan of the outputs (mtf_plan), the slice rule (mtf_slices, mtf_slice), a ray about its centre
// (mtf_stage_ray), the phase with its fp32 phasor (mtf_phasor) and the tail (mtf_finish) are the core's, in prt_mtf.hpp.
#pragma once

#include <type_traits>
#include <vector>

enum { MTFG_MAX_PARAMETERS = 16, MTFG_RECORD = 7 };  // (a group's record: MTFG_RECORD + 3 K doubles)
static const int kMtfgBlock = 256;                 // threads of a sum workgroup
static const int kMtfgTile = 128;                  // rays of its LDS tile
static const int kMtfgOut = 2;                     // outputs a thread owns
static const int kMtfgParams = 8;                  // parameters of a chunk at most (fp64 accumulators in registers)
static const int kMtfgChunk = 1024;                // selected rows of a centre chunk
static const int kMtfgMinSlice = 2048;             // selected rows a sum slice holds at least (while the group has them)
static const int kMtfgMaxSlices = 256;             // slices of a group at most (the fold walks them in series)
static const int kMtfgQuantities = MTFG_MAX_PARAMETERS + 2;  // the slab holds OTF, K parameters and the focus: sized for 16
static const size_t kMtfgSlabBytes = 256u << 20;   // cap on the (slice, quantity, output) partial sums
static_assert(kMtfgMinSlice == kMtfMinSlice && kMtfgMaxSlices == kMtfMaxSlices && kMtfgSlabBytes == kMtfSlabBytes,
              "the slices are the MTF's: mtf_slices and mtf_plan apply its constants");

struct MtfgPar { double dp1, dp2, ds1, ds2; };     // (32 bytes: two 16-byte LDS reads)

// the state of selected row `slot`: 0 kept, 1 left out by the MTF's rule (or a row number outside the frame), 2 not
// followed (a Jacobian or slope entry that is not finite); r is filled for a row that passes the MTF's rule
__device__ __forceinline__ int mtfg_ray(const double* __restrict__ rows, int64_t ld, int64_t n_rows,
                                        const int64_t* __restrict__ selected, int64_t n_selected, int64_t slot,
                                        const MtfAxes& ax, int weight_column, const double* __restrict__ jacobian,
                                        const double* __restrict__ slopes, int K, MtfRaw& r) {
  const int64_t j = selected[slot];
  if (j < 0 || j >= n_rows || !mtf_ray(rows, ld, j, ax, weight_column, r)) return 1;
  bool ok = true;
  for (int k = 0; k < 3 * K; ++k)
    ok = ok && fabs(jacobian[(int64_t)k * n_selected + slot]) < PRT_INF && fabs(slopes[(int64_t)k * n_selected + slot]) < PRT_INF;
  return ok ? 0 : 2;
}

// per (group, chunk), 7 + 3 K doubles: [0] kept [1] missed [2] unfollowed [3] sum w [4..6] sum w Q [7 + 3 k + c] sum w
// dQ_k.c -- each thread over its strided rows in order, then a fixed tree: the lanes of a wave pairwise by shuffles
// (32, 16, ... 1 apart), then the waves in order
__global__ void __launch_bounds__(kMtfgBlock)
k_mtfg_centre(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ selected,
              int64_t n_selected, int n_groups, const int64_t* __restrict__ group_first,
              const int64_t* __restrict__ chunk_start, MtfAxes ax, int weight_column,
              const double* __restrict__ jacobian, const double* __restrict__ slopes, int K, double* __restrict__ slab) {
  __shared__ double weight[kMtfgChunk];  // the row's weight if it is kept, -1 missed, -2 unfollowed
  __shared__ double red[MTFG_RECORD + 3 * MTFG_MAX_PARAMETERS][kMtfgBlock / 64];
  const int t = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int g = mtf_owner(chunk_start, n_groups, chunk);
  if (g < 0) return;
  const int64_t lo = group_first[g] + (chunk - chunk_start[g]) * kMtfgChunk;
  const int64_t hi = lo + kMtfgChunk < group_first[g + 1] ? lo + kMtfgChunk : group_first[g + 1];
  for (int64_t r = lo + t; r < hi; r += kMtfgBlock) {
    MtfRaw ray;
    const int state = mtfg_ray(rows, ld, n_rows, selected, n_selected, r, ax, weight_column, jacobian, slopes, K, ray);
    weight[r - lo] = state == 0 ? ray.w : -(double)state;
  }
  const int n_q = MTFG_RECORD + 3 * K;
  for (int q = 0; q < n_q; ++q) {
    double s = 0.0;
    for (int64_t r = lo + t; r < hi; r += kMtfgBlock) {  // (the thread's own entries of weight: no barrier needed)
      const double w = weight[r - lo];
      if (q < 3) {
        s += (q == 0 ? w >= 0.0 : w == -(double)q) ? 1.0 : 0.0;
      } else if (w >= 0.0) {
        if (q == 3) s += w;
        else if (q < 7) s = fma(w, rows[(int64_t)(PRT_COL_X1 + q - 4) * ld + selected[r]], s);
        else s = fma(w, jacobian[(int64_t)(q - 7) * n_selected + r], s);
      }
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((t & 63) == 0) red[q][t >> 6] = s;
  }
  __syncthreads();
  if (t < n_q) {
    double s = red[t][0];
    for (int w = 1; w < kMtfgBlock / 64; ++w) s += red[t][w];
    slab[chunk * n_q + t] = s;
  }
}

// per (group, quantity), a wave each: the group's chunks in a fixed order -- lane l takes chunks l, l + 64, ..., then the
// lanes are added pairwise -- into record_out, still in the slab's order (k_mtfg_record puts it right)
__global__ void __launch_bounds__(64)
k_mtfg_centre_fold(int n_groups, int K, const int64_t* __restrict__ chunk_start, const double* __restrict__ slab,
                   double* __restrict__ record_out) {
  const int n_q = MTFG_RECORD + 3 * K;
  const int g = blockIdx.x / n_q, q = blockIdx.x - g * n_q;
  double s = 0.0;
  for (int64_t c = chunk_start[g] + threadIdx.x; c < chunk_start[g + 1]; c += 64) s += slab[c * n_q + q];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if (threadIdx.x == 0) record_out[(size_t)g * n_q + q] = s;
}

// per group: record_out from the slab's order (counts, sum w, sum w Q, sum w dQ) to C (3), [3] sum w (k_mtfg_fold), rays
// used, missed, unfollowed, dC_k; the centre is the centroid or the given reference
__global__ void __launch_bounds__(PRT_BLOCK)
k_mtfg_record(int n_groups, int K, const double* __restrict__ reference, double* __restrict__ centre,
              double* __restrict__ record_out) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  const int n_q = MTFG_RECORD + 3 * K;
  double* const out = record_out + (size_t)g * n_q;
  const double counts[3] = {out[0], out[1], out[2]}, sw = out[3], sq[3] = {out[4], out[5], out[6]};
  for (int k = 0; k < 3; ++k) {
    const double c = reference ? reference[3 * g + k] : sq[k] / sw;  // (no rays, or sum w = 0: NaN)
    centre[3 * g + k] = c;
    out[k] = c;
    out[4 + k] = counts[k];
  }
  for (int k = 0; k < 3 * K; ++k) out[7 + k] = out[7 + k] / sw;
}

// per selected row: d = Q - C, ua = u.a / |u|, s = (u.e1, u.e2) / u.a, p = (d.e1, d.e2) - s (d.a); per parameter
// ds = ((du.e1, du.e2) - s (du.a)) / ua, dp = (dQ.e1, dQ.e2) - s (dQ.a) - ds (d.a)
__global__ void __launch_bounds__(kMtfgBlock)
k_mtfg_stage(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ selected,
             int64_t n_selected, int n_groups, const int64_t* __restrict__ group_first, const double* __restrict__ centre,
             MtfAxes ax, int weight_column, const double* __restrict__ jacobian, const double* __restrict__ slopes, int K,
             MtfRay* __restrict__ stage, MtfgPar* __restrict__ stage_par) {
  const int64_t r = (int64_t)blockIdx.x * kMtfgBlock + threadIdx.x;
  if (r >= n_selected) return;
  MtfRaw ray;
  if (mtfg_ray(rows, ld, n_rows, selected, n_selected, r, ax, weight_column, jacobian, slopes, K, ray) != 0) {
    stage[r] = MtfRay{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < K; ++k) stage_par[(int64_t)k * n_selected + r] = MtfgPar{0.0, 0.0, 0.0, 0.0};
    return;
  }
  const int g = mtf_owner(group_first, n_groups, r);
  const double c[3] = {centre[3 * g], centre[3 * g + 1], centre[3 * g + 2]};
  double s1, s2, da, ua;
  stage[r] = mtf_stage_ray(ray, c, ax, s1, s2, da, ua);
  const double unit_a = ua / sqrt(ray.u[0] * ray.u[0] + ray.u[1] * ray.u[1] + ray.u[2] * ray.u[2]);
  for (int k = 0; k < K; ++k) {
    double dq[3], du[3];
    for (int i = 0; i < 3; ++i) {
      dq[i] = jacobian[(int64_t)(3 * k + i) * n_selected + r];
      du[i] = slopes[(int64_t)(3 * k + i) * n_selected + r];
    }
    const double ua_k = du[0] * ax.a[0] + du[1] * ax.a[1] + du[2] * ax.a[2];
    const double ds1 = ((du[0] * ax.e1[0] + du[1] * ax.e1[1] + du[2] * ax.e1[2]) - s1 * ua_k) / unit_a;
    const double ds2 = ((du[0] * ax.e2[0] + du[1] * ax.e2[1] + du[2] * ax.e2[2]) - s2 * ua_k) / unit_a;
    const double qa_k = dq[0] * ax.a[0] + dq[1] * ax.a[1] + dq[2] * ax.a[2];
    const double dp1 = ((dq[0] * ax.e1[0] + dq[1] * ax.e1[1] + dq[2] * ax.e1[2]) - s1 * qa_k) - ds1 * da;
    const double dp2 = ((dq[0] * ax.e2[0] + dq[1] * ax.e2[1] + dq[2] * ax.e2[2]) - s2 * qa_k) - ds2 * da;
    stage_par[(int64_t)k * n_selected + r] = MtfgPar{dp1, dp2, ds1, ds2};
  }
}

// A workgroup is `lanes` lanes of kMtfgBlock / lanes threads, as in k_mtf_sum; each thread owns kMtfgOut outputs of the
// tile and, for each, the accumulators of P parameters [first, first + P) (those past K are zeros that are not stored).
// The workgroup whose chunk starts at parameter 0 also sums the OTF, the focus derivative (g = k.s) and sum w.
// slab: (slice, quantity, output, 2), quantity 0 the OTF, 1 + k parameter k, K + 1 the focus.
template <int P>
__global__ void __launch_bounds__(kMtfgBlock)
k_mtfg_sum(int n_groups, const int64_t* __restrict__ slice_start, const int64_t* __restrict__ group_first,
           const MtfRay* __restrict__ stage, const MtfgPar* __restrict__ stage_par, int64_t n_selected, int K,
           int first_parameter, const double* __restrict__ table, const double* __restrict__ focus, int n_k,
           int64_t n_out, int lanes, double* __restrict__ slab, double* __restrict__ weight_slab) {
  __shared__ MtfRay tile[kMtfgTile];
  __shared__ MtfgPar tile_par[P][kMtfgTile];
  __shared__ double fold[2][kMtfgBlock];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int g = mtf_owner(slice_start, n_groups, s);
  if (g < 0) return;
  const int first = first_parameter + (int)blockIdx.z * P;
  const bool head = first == 0;
  const int threads = kMtfgBlock / lanes, lane = t / threads, me = t - lane * threads;
  double kc[kMtfgOut], ks[kMtfgOut], kcd[kMtfgOut], ksd[kMtfgOut];
  double re[kMtfgOut], im[kMtfgOut], fre[kMtfgOut], fim[kMtfgOut], are[kMtfgOut][P], aim[kMtfgOut][P];
#pragma unroll
  for (int q = 0; q < kMtfgOut; ++q) {
    const int64_t o = (int64_t)blockIdx.y * threads * kMtfgOut + q * threads + me;
    const int64_t oo = o < n_out ? o : 0;
    const int64_t f = oo / n_k, k = oo - f * n_k;
    kc[q] = table[2 * k];
    ks[q] = table[2 * k + 1];
    kcd[q] = kc[q] * focus[f];
    ksd[q] = ks[q] * focus[f];
    re[q] = im[q] = fre[q] = fim[q] = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) are[q][j] = aim[q][j] = 0.0;
  }
  double sw = 0.0;
  int64_t lo, hi;
  mtf_slice(slice_start, group_first, group_first[g + 1] - group_first[g], g, s, lo, hi);
  for (int64_t base = lo; base < hi; base += kMtfgTile) {
    const int count = hi - base < kMtfgTile ? (int)(hi - base) : kMtfgTile;
    __syncthreads();  // (the previous tile is read)
    if (t < count) tile[t] = stage[base + t];
    for (int item = t; item < P * kMtfgTile; item += kMtfgBlock) {
      const int j = item / kMtfgTile, r = item - j * kMtfgTile;
      if (r < count)
        tile_par[j][r] = first + j < K ? stage_par[(int64_t)(first + j) * n_selected + base + r] : MtfgPar{0.0, 0.0, 0.0, 0.0};
    }
    __syncthreads();
    for (int r = lane; r < count; r += lanes) {
      const MtfRay ray = tile[r];
      sw += ray.w;
#pragma unroll
      for (int q = 0; q < kMtfgOut; ++q) {
        // the phase and its phasor as k_mtf_sum has them (mtf_phasor); the first-order correction for what the
        // conversion to fp32 drops is folded into the phasor once: (c', sn') = (c - theta sn, sn + theta c)
        double c, sn;
        const double theta = mtf_phasor(kc[q], ks[q], kcd[q], ksd[q], ray, c, sn);
        const double wc = ray.w * fma(-theta, sn, c), ws = ray.w * fma(theta, c, sn);
        if (head) {
          re[q] += wc;
          im[q] += ws;
          const double gf = fma(kc[q], ray.s1, ks[q] * ray.s2);
          fre[q] = fma(gf, ws, fre[q]);
          fim[q] = fma(gf, wc, fim[q]);
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const MtfgPar d = tile_par[j][r];
          const double gk = fma(kc[q], d.dp1, fma(ks[q], d.dp2, fma(kcd[q], d.ds1, ksd[q] * d.ds2)));
          are[q][j] = fma(gk, ws, are[q][j]);
          aim[q][j] = fma(gk, wc, aim[q][j]);
        }
      }
    }
  }
  // one accumulator pair after another: the lanes' sums added in lane order through LDS, then stored by lane 0
  auto finish = [&](double a, double b, int quantity, int q) {
    if (lanes > 1) {
      __syncthreads();
      fold[0][t] = a;
      fold[1][t] = b;
      __syncthreads();
      if (lane == 0)
        for (int l = 1; l < lanes; ++l) {
          a += fold[0][l * threads + me];
          b += fold[1][l * threads + me];
        }
    }
    const int64_t o = (int64_t)blockIdx.y * threads * kMtfgOut + q * threads + me;
    if (lane == 0 && o < n_out) {
      double* p = slab + (((size_t)s * (K + 2) + quantity) * n_out + o) * 2;
      p[0] = a;
      p[1] = b;
    }
  };
#pragma unroll
  for (int q = 0; q < kMtfgOut; ++q) {
    if (head) {
      finish(re[q], im[q], 0, q);
      finish(fre[q], fim[q], K + 1, q);
    }
#pragma unroll
    for (int j = 0; j < P; ++j)
      if (first + j < K) finish(are[q][j], aim[q][j], 1 + first + j, q);
  }
  if (head && blockIdx.y == 0) {
    __syncthreads();
    fold[0][t] = sw;
    __syncthreads();
    if (t == 0) {
      for (int l = 1; l < lanes; ++l) sw += fold[0][l * threads];
      weight_slab[s] = sw;
    }
  }
}

// per (group, quantity, output): the slices in slice order.  OTF = (sum w cos, -sum w sin) / sum w; a derivative is
// -2 pi i sum w g (cos - i sin) / sum w = -2 pi (sum w g sin, sum w g cos) / sum w.  dotf_out: (group, K + 1, output, 2)
__global__ void __launch_bounds__(PRT_BLOCK)
k_mtfg_fold(int n_groups, int K, int64_t n_out, const int64_t* __restrict__ slice_start, const double* __restrict__ slab,
            const double* __restrict__ weight_slab, double* __restrict__ otf_out, double* __restrict__ dotf_out,
            double* __restrict__ record_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * (K + 2) * n_out) return;
  const int g = (int)(item / ((K + 2) * n_out));
  const int quantity = (int)((item - (int64_t)g * (K + 2) * n_out) / n_out);
  const int64_t o = item - ((int64_t)g * (K + 2) + quantity) * n_out;
  double a = 0.0, b = 0.0, sw = 0.0;
  for (int64_t s = slice_start[g]; s < slice_start[g + 1]; ++s) {
    const double* p = slab + (((size_t)s * (K + 2) + quantity) * n_out + o) * 2;
    a += p[0];
    b += p[1];
    sw += weight_slab[s];
  }
  const double two_pi = 6.283185307179586;
  if (quantity == 0) {  // (a group without rays, or with sum w = 0: 0 / 0, NaN)
    otf_out[((int64_t)g * n_out + o) * 2] = a / sw;
    otf_out[((int64_t)g * n_out + o) * 2 + 1] = -b / sw;
    if (o == 0) record_out[(size_t)g * (MTFG_RECORD + 3 * K) + 3] = sw;
  } else {
    double* p = dotf_out + (((int64_t)g * (K + 1) + quantity - 1) * n_out + o) * 2;
    p[0] = -two_pi * a / sw;
    p[1] = -two_pi * b / sw;
  }
}

// ---- the staging of prt_frame_mtf_gradient and prt_frame_mtf_tolerance: a group's share follows from its own count of
// selected rows and max_slices; a pass makes it, refuses what is too large, allocates its scratch and calls mtfg_stage
struct MtfgStaging {
  std::vector<int64_t> starts;           // group, chunk and slice starts, n_groups + 1 each (they outlive their copy)
  int64_t chunk_grid, slice_grid, centre_bytes;  // chunks and slices of all groups; the centre slab, first in the scratch
  int64_t *d_group, *d_chunk, *d_slice;  // the starts in the workspace, then
  double *centre, *rest;                 // the centres (n_groups, 3), then what is the pass's own
  MtfgStaging(const int64_t* group_first, int n_groups, int K, int64_t max_slices, void* workspace)
      : starts(3 * ((size_t)n_groups + 1)) {
    int64_t *const h_group = starts.data(), *const h_chunk = h_group + n_groups + 1, *const h_slice = h_chunk + n_groups + 1;
    for (int g = 0; g <= n_groups; ++g) h_group[g] = group_first[g];
    for (int g = 0; g < n_groups; ++g) {  // (h_chunk[0] and h_slice[0] are 0)
      const int64_t count = group_first[g + 1] - group_first[g];
      h_chunk[g + 1] = h_chunk[g] + (count + kMtfgChunk - 1) / kMtfgChunk;
      h_slice[g + 1] = h_slice[g] + mtf_slices(count, max_slices);
    }
    chunk_grid = h_chunk[n_groups], slice_grid = h_slice[n_groups];
    centre_bytes = std::max<int64_t>(chunk_grid, 1) * (MTFG_RECORD + 3 * K) * (int64_t)sizeof(double);
    d_group = (int64_t*)workspace, d_chunk = d_group + (n_groups + 1), d_slice = d_chunk + (n_groups + 1);
    centre = (double*)(d_slice + (n_groups + 1)), rest = centre + 3 * (size_t)n_groups;
  }
};
// the starts copied, then the four staging kernels; record: (n_groups, MTFG_RECORD + 3 K); the caller refuses the sizes
static int mtfg_stage(const MtfgStaging& s, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                      int64_t n_selected, int n_groups, int weight_column, const double* jacobian, const double* slopes,
                      int K, const double* reference, const MtfPlan& plan, double* centre_slab, double* record,
                      MtfRay* stage, MtfgPar* stage_par, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(s.d_group, s.starts.data(), s.starts.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
  if (s.chunk_grid)
    hipLaunchKernelGGL(k_mtfg_centre, dim3((unsigned)s.chunk_grid), dim3(kMtfgBlock), 0, st, rows, ld, n_rows, selected,
                       n_selected, n_groups, s.d_group, s.d_chunk, plan.ax, weight_column, jacobian, slopes, K, centre_slab);
  hipLaunchKernelGGL(k_mtfg_centre_fold, dim3((unsigned)(n_groups * (MTFG_RECORD + 3 * K))), dim3(64), 0, st, n_groups, K,
                     s.d_chunk, centre_slab, record);
  hipLaunchKernelGGL(k_mtfg_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     n_groups, K, reference, s.centre, record);
  if (n_selected)
    hipLaunchKernelGGL(k_mtfg_stage, dim3((unsigned)((n_selected + kMtfgBlock - 1) / kMtfgBlock)), dim3(kMtfgBlock), 0, st,
                       rows, ld, n_rows, selected, n_selected, n_groups, s.d_group, s.centre, plan.ax, weight_column,
                       jacobian, slopes, K, stage, stage_par);
  return PRT_OK;
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t prt_frame_mtf_gradient_workspace_bytes(int64_t n_selected, int n_groups, int n_parameters,
                                                          int n_frequencies, int n_azimuths, int n_focus) {
  if (n_selected < 0 || n_groups < 1 || n_groups > 65535 || n_parameters < 1 || n_parameters > MTFG_MAX_PARAMETERS ||
      n_frequencies < 1 || n_frequencies > MTF_MAX_FREQUENCIES || n_azimuths < 1 || n_azimuths > MTF_MAX_AZIMUTHS ||
      n_focus < 1 || n_focus > MTF_MAX_FOCUS)
    return PRT_ERR_ARG;
  // group, chunk and slice starts (n_groups + 1 each), centres, the (kc, ks) table and the planes, the staged rays
  return (3 * ((int64_t)n_groups + 1) + 3 * (int64_t)n_groups) * 8 +
         (int64_t)(2 * n_frequencies * n_azimuths + n_focus) * 8 +
         n_selected * (int64_t)(sizeof(MtfRay) + (size_t)n_parameters * sizeof(MtfgPar)) + 64;
}

extern "C" int prt_frame_mtf_gradient(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                                      int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                                      const double* jacobian, const double* slopes, int n_parameters,
                                      const double* reference, const double* axes, const double* frequencies,
                                      int n_frequencies, const double* azimuths_deg, int n_azimuths, const double* focus,
                                      int n_focus, double* otf_out, double* dotf_out, double* record_out, void* workspace,
                                      void* stream) {
  // (everything is checked before a device is touched)
  const int K = n_parameters;
  if (n_rows < 0 || ld < n_rows || n_selected < 0 || n_groups < 1 || n_groups > 65535 || !otf_out || !dotf_out ||
      !record_out || !workspace || !axes || !group_first || (n_rows && !rows))
    return fail(PRT_ERR_ARG, "mtf_gradient: bad buffers");
  if (K < 1 || K > MTFG_MAX_PARAMETERS) return fail(PRT_ERR_ARG, "mtf_gradient: 1 to 16 parameters");
  if (n_selected && (!selected || !jacobian || !slopes))
    return fail(PRT_ERR_ARG, "mtf_gradient: selected, jacobian and slopes where rows are selected");
  if (int bad = selection_check("mtf_gradient", n_rows, n_selected, group_first, n_groups, weight_column)) return bad;
  // the slab is sized for 16 parameters whatever K is, so that the slices do not follow K
  MtfPlan plan;
  int rc = mtf_plan("mtf_gradient", frequencies, n_frequencies, azimuths_deg, n_azimuths, focus, n_focus, axes, n_groups,
                    kMtfgQuantities * 16, kMtfgOut, kMtfgBlock, plan);
  if (rc) return rc;
  const int n_k = plan.n_k, lanes = plan.lanes;
  const int64_t n_out = plan.n_out, tiles = plan.tiles;
  const MtfgStaging staging(group_first, n_groups, K, plan.max_slices, workspace);
  const int64_t slice_grid = staging.slice_grid;
  if (staging.chunk_grid > 0x7fffffff || slice_grid > 0x7fffffff || tiles > 65535 ||
      (n_selected + kMtfgBlock - 1) / kMtfgBlock > 0x7fffffff)
    return fail(PRT_ERR_ARG, "mtf_gradient: too many rows or outputs for one launch");
  rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace after the staging's head (prt_frame_mtf_gradient_workspace_bytes)
  const int64_t *d_group = staging.d_group, *d_slice = staging.d_slice;
  double* table = staging.rest;
  double* planes = table + 2 * (size_t)n_k;
  MtfRay* stage = (MtfRay*)(((uintptr_t)(planes + n_focus) + 31) & ~(uintptr_t)31);
  MtfgPar* stage_par = (MtfgPar*)(stage + n_selected);
  const size_t centre_bytes = staging.centre_bytes, weight_bytes = (size_t)slice_grid * sizeof(double);
  const size_t slab_bytes = (size_t)slice_grid * (K + 2) * n_out * 2 * sizeof(double);
  char* scratch = nullptr;
  HIP_TRY(hipMallocAsync((void**)&scratch, centre_bytes + weight_bytes + slab_bytes, st));
  double* weight_slab = (double*)(scratch + centre_bytes);
  double* slab = (double*)(scratch + centre_bytes + weight_bytes);
  HIP_TRY(hipMemcpyAsync(table, plan.host.data(), plan.host.size() * sizeof(double), hipMemcpyHostToDevice, st));
  rc = mtfg_stage(staging, rows, ld, n_rows, selected, n_selected, n_groups, weight_column, jacobian, slopes, K, reference,
                  plan, (double*)scratch, record_out, stage, stage_par, st);
  if (rc) return rc;
  // whole chunks of kMtfgParams parameters in one launch, then the rest in the smallest instantiation that holds it
  const int whole = K / kMtfgParams, rest = K - whole * kMtfgParams;
  auto sum = [&](auto chunk, int chunks, int first) {
    hipLaunchKernelGGL(k_mtfg_sum<decltype(chunk)::value>, dim3((unsigned)slice_grid, (unsigned)tiles, (unsigned)chunks),
                       dim3(kMtfgBlock), 0, st, n_groups, d_slice, d_group, stage, stage_par, n_selected, K, first, table,
                       planes, n_k, n_out, lanes, slab, weight_slab);
  };
  if (whole) sum(std::integral_constant<int, kMtfgParams>(), whole, 0);
  if (rest > 4) sum(std::integral_constant<int, 8>(), 1, whole * kMtfgParams);
  else if (rest > 2) sum(std::integral_constant<int, 4>(), 1, whole * kMtfgParams);
  else if (rest == 2) sum(std::integral_constant<int, 2>(), 1, whole * kMtfgParams);
  else if (rest == 1) sum(std::integral_constant<int, 1>(), 1, whole * kMtfgParams);
  hipLaunchKernelGGL(k_mtfg_fold,
                     dim3((unsigned)(((int64_t)n_groups * (K + 2) * n_out + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK),
                     0, st, n_groups, K, n_out, d_slice, slab, weight_slab, otf_out, dotf_out, record_out);
  return mtf_finish(st, scratch);  // (it drains the stream: the host starts outlive their copy, too)
}

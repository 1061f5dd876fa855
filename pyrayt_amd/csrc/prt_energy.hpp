// prt_energy.hpp -- geometric encircled / ensquared energy of the frame through focus, and its inverse, on the device
// (DESIGN.md section 4.5).  Like the MTF it needs only each ray's end point and direction at the detector.  Definitions:
// include/prt.h.
//
// The MTF's staging pass runs as it is (mtf_stage_rows of prt_mtf.hpp: k_mtf_count / offsets / starts / scatter /
// centre / record / stage): per group, in row order, each ray's (p1, p2, s1, s2, w) about the group's centre.  Then
//   k_energy_centre   per (group, chunk of 4096 rays): sum w, sum w p, sum w s in a fixed tree; the chunk's largest
//                     weight into the group's w_max (one integer atomic max on the double's bits per workgroup)
//   k_energy_record   per group: the chunks folded in order into pbar, sbar and sum w; the shift 62 - E - B; the record
//   k_energy_scale    per (group, chunk): q_r = floor(ldexp(w_r, shift)) beside the staged rays; W = sum q (integer
//                     atomics, one per workgroup)
//   k_energy_curve    per (ray slice of a group, plane tile): d of every ray at every plane of the tile, searched in the
//                     radii (LDS), q added to a (plane, radius bin) window of uint64 in LDS (ds_add_u64); non-zero
//                     bins flushed with 64-bit integer global atomics
//   k_energy_finish   per (group, plane): the bins prefix-summed and divided by W
//   k_energy_begin    per (group, plane, fraction): the threshold T_k and an empty prefix
//   k_energy_select   one pass of the MSD radix select on the bit image of d: per (ray slice, plane), per fraction of
//                     the tile, a ray whose key matches the fraction's prefix adds q to the fraction's digit window in
//                     LDS; the windows flushed with integer global atomics
//   k_energy_digit    per (group, plane, fraction): the window scanned, the digit where the running sum first reaches
//                     the residual threshold appended to the prefix, what lay below subtracted, the window zeroed;
//                     after the last pass the prefix is the radius
// Every sum that decides an output is an integer sum: exact in any order.  The only float sums (pbar, sbar, sum w) have
// a fixed order.  Every partition depends on a group's count of rays used and on the output counts, never on n_rows.
#pragma once

enum { ENERGY_MAX_RADII = 4096, ENERGY_MAX_FRACTIONS = 16, ENERGY_MAX_FOCUS = 256, ENERGY_RECORD = 10 };
static const int kEnergyBlock = 256;
static const int kEnergyWindow = 4096;          // (plane, radius bin) tallies of a curve workgroup: 32 KiB beside the radii
static const int kEnergyDigits = 2048;          // tallies of one fraction's digit window: 16 KiB
static const int kEnergyFractionTile = 4;       // digit windows of a select workgroup: 64 KiB, two workgroups a CU
static const int kEnergyPasses = 6;             // the 63 bits of a non-negative double, most significant digit first
static const int kEnergyWidth[kEnergyPasses] = {11, 11, 11, 10, 10, 10};
static const int kEnergyLow[kEnergyPasses] = {52, 41, 30, 20, 10, 0};
static const size_t kEnergySlabBytes = 256u << 20;  // cap on the radius bins, and on the digit windows

typedef unsigned long long u64;

// d of a staged ray at the plane shifted by delta, about c: x = (p + delta s) - c, products and sums rounded one by
// one in this order; a coordinate that is NaN (c itself overflowed) gives +inf
__device__ __forceinline__ double energy_distance(const MtfRay& r, double delta, double c1, double c2, int shape) {
  const double x1 = (r.p1 + delta * r.s1) - c1, x2 = (r.p2 + delta * r.s2) - c2;
  if (x1 != x1 || x2 != x2) return PRT_INF;
  const double a1 = fabs(x1), a2 = fabs(x2);
  if (shape == PRT_ENERGY_CIRCLE) return sqrt(x1 * x1 + x2 * x2);
  if (shape == PRT_ENERGY_SQUARE) return a1 > a2 ? a1 : a2;
  return shape == PRT_ENERGY_SLIT_E2 ? a1 : a2;
}

// the power-of-two rule that makes the weights integers: with w_max = f 2^E (0.5 <= f < 1; its bit image is given) and
// B = bit_length(count), the shift is 62 - E - B and q = floor(ldexp(w, shift)) -- count such q sum to less than 2^62
__device__ __forceinline__ int energy_shift(u64 w_max_bits, long long count) {
  int e = 0;
  frexp(__longlong_as_double((long long)w_max_bits), &e);
  return 62 - e - (64 - __clzll(count));
}
__device__ __forceinline__ u64 energy_quantum(double w, int shift) { return (u64)floor(ldexp(w, shift)); }

// per (group, chunk): [0] sum w  [1..2] sum w p  [3..4] sum w s -- each thread over its strided rays in order, then a
// fixed tree; the largest weight of the chunk into w_max[g]
__global__ void __launch_bounds__(kEnergyBlock)
k_energy_centre(int n_groups, const int64_t* __restrict__ chunk_start, const int64_t* __restrict__ bucket_total,
                const int64_t* __restrict__ bucket_start, const MtfRay* __restrict__ stage, double* __restrict__ slab,
                u64* __restrict__ w_max) {
  __shared__ double red[6][kEnergyBlock];
  const int t = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int g = mtf_owner(chunk_start, n_groups, chunk);
  if (g < 0) return;
  int64_t lo, hi;
  mtf_chunk(chunk_start, bucket_total, bucket_start, g, chunk, lo, hi);
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, top = 0.0;
  for (int64_t r = lo + t; r < hi; r += kEnergyBlock) {
    const MtfRay ray = stage[r];
    s[0] += ray.w;
    s[1] = fma(ray.w, ray.p1, s[1]);
    s[2] = fma(ray.w, ray.p2, s[2]);
    s[3] = fma(ray.w, ray.s1, s[3]);
    s[4] = fma(ray.w, ray.s2, s[4]);
    top = ray.w > top ? ray.w : top;
  }
  for (int k = 0; k < 5; ++k) red[k][t] = s[k];
  red[5][t] = top;
  sort_tree(red, t, [](int k, double& a, double b) { a = k < 5 ? a + b : (b > a ? b : a); });  // (five sums, one max)
  if (t < 5) slab[chunk * 5 + t] = red[t][0];
  // (weights are >= 0: the order of their bit images is their own)
  if (t == 5 && red[5][0] > 0.0) atomicMax(w_max + g, (u64)__double_as_longlong(red[5][0]));
}

// per group: pbar, sbar and sum w from the chunks in order; shift = 62 - E - B; record_out
__global__ void __launch_bounds__(PRT_BLOCK)
k_energy_record(int n_groups, const int64_t* __restrict__ chunk_start, const double* __restrict__ slab,
                const double* __restrict__ centre, const int64_t* __restrict__ bucket_total,
                const u64* __restrict__ missed, const u64* __restrict__ w_max, double* __restrict__ centroid,
                int* __restrict__ shift, double* __restrict__ record_out) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t q = chunk_start[g]; q < chunk_start[g + 1]; ++q)
    for (int k = 0; k < 5; ++k) s[k] += slab[q * 5 + k];
  double* r = record_out + (size_t)g * ENERGY_RECORD;
  for (int k = 0; k < 3; ++k) r[k] = centre[3 * g + k];
  for (int k = 0; k < 4; ++k) {
    const double mean = s[1 + k] / s[0];  // (no rays, or sum w = 0: NaN)
    centroid[4 * g + k] = mean;
    r[3 + k] = mean;
  }
  r[7] = s[0];
  r[8] = (double)bucket_total[g];
  r[9] = (double)missed[g];
  shift[g] = energy_shift(w_max[g], (long long)bucket_total[g]);
}

// per (group, chunk): q_r = (uint64) floor(ldexp(w_r, shift)); W[g] += the chunk's sum
__global__ void __launch_bounds__(kEnergyBlock)
k_energy_scale(int n_groups, const int64_t* __restrict__ chunk_start, const int64_t* __restrict__ bucket_total,
               const int64_t* __restrict__ bucket_start, const MtfRay* __restrict__ stage, const int* __restrict__ shift,
               u64* __restrict__ q, u64* __restrict__ total) {
  __shared__ u64 red[1][kEnergyBlock];
  const int t = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int g = mtf_owner(chunk_start, n_groups, chunk);
  if (g < 0) return;
  int64_t lo, hi;
  mtf_chunk(chunk_start, bucket_total, bucket_start, g, chunk, lo, hi);
  const int by = shift[g];
  u64 mine = 0;
  for (int64_t r = lo + t; r < hi; r += kEnergyBlock) {
    const u64 v = energy_quantum(stage[r].w, by);
    q[r] = v;
    mine += v;
  }
  red[0][t] = mine;
  sort_tree(red, t);
  if (t == 0 && red[0][0]) atomicAdd(total + g, red[0][0]);
}

// per (ray slice, plane tile): bins[(g, plane, j)] += q of the rays with R_(j-1) < d <= R_j
__global__ void __launch_bounds__(kEnergyBlock)
k_energy_curve(int n_groups, const int64_t* __restrict__ slice_start, const int64_t* __restrict__ bucket_total,
               const int64_t* __restrict__ bucket_start, const MtfRay* __restrict__ stage, const u64* __restrict__ q,
               const u64* __restrict__ total, const double* __restrict__ centroid, const double* __restrict__ focus,
               int n_focus, int planes_per_tile, int shape, int follow, const double* __restrict__ radii, int n_radii,
               u64* __restrict__ bins) {
  __shared__ double edge[ENERGY_MAX_RADII];
  __shared__ u64 window[kEnergyWindow];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int g = mtf_owner(slice_start, n_groups, s);
  if (g < 0 || total[g] == 0) return;
  const int f0 = blockIdx.y * planes_per_tile;
  const int planes = n_focus - f0 < planes_per_tile ? n_focus - f0 : planes_per_tile;
  const int cells = planes * n_radii;  // (<= kEnergyWindow: the host sized the tile)
  for (int k = t; k < n_radii; k += kEnergyBlock) edge[k] = radii[k];
  for (int k = t; k < cells; k += kEnergyBlock) window[k] = 0;
  __syncthreads();
  const double pb1 = follow ? centroid[4 * g] : 0.0, pb2 = follow ? centroid[4 * g + 1] : 0.0;
  const double sb1 = follow ? centroid[4 * g + 2] : 0.0, sb2 = follow ? centroid[4 * g + 3] : 0.0;
  int64_t lo, hi;
  mtf_slice(slice_start, bucket_start, bucket_total[g], g, s, lo, hi);  // (the MTF's slices)
  for (int64_t r = lo + t; r < hi; r += kEnergyBlock) {
    const MtfRay ray = stage[r];
    const u64 weight = q[r];
    if (!weight) continue;
    for (int f = 0; f < planes; ++f) {
      const double delta = focus[f0 + f];
      const double c1 = follow ? pb1 + delta * sb1 : 0.0, c2 = follow ? pb2 + delta * sb2 : 0.0;
      const double d = energy_distance(ray, delta, c1, c2, shape);
      int a = 0, b = n_radii;  // the first j with d <= R_j
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (edge[mid] < d) a = mid + 1; else b = mid;
      }
      if (a < n_radii) atomicAdd(&window[f * n_radii + a], weight);
    }
  }
  __syncthreads();
  for (int k = t; k < cells; k += kEnergyBlock) {
    const u64 v = window[k];
    if (v) atomicAdd(bins + ((size_t)g * n_focus + f0) * n_radii + k, v);
  }
}

// per (group, plane): EE(R_j) = (sum of the bins up to j) / W; the select's radius is NaN where W = 0
__global__ void __launch_bounds__(PRT_BLOCK)
k_energy_finish(int n_groups, int n_focus, int n_radii, const u64* __restrict__ bins, const u64* __restrict__ total,
                double* __restrict__ energy_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * n_focus) return;
  const u64 all = total[item / n_focus];
  u64 run = 0;
  for (int j = 0; j < n_radii; ++j) {
    run += bins[item * n_radii + j];
    energy_out[item * n_radii + j] = all ? (double)run / (double)all : __longlong_as_double(0x7ff8000000000000ll);
  }
}

// per (group, plane, fraction): state = (prefix 0, residual T_k); radius_out NaN where W = 0
__global__ void __launch_bounds__(PRT_BLOCK)
k_energy_begin(int n_groups, int n_focus, int n_fractions, const double* __restrict__ fractions,
               const u64* __restrict__ total, u64* __restrict__ state, double* __restrict__ radius_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * n_focus * n_fractions) return;
  const u64 all = total[item / ((int64_t)n_focus * n_fractions)];
  u64 need = (u64)ceil(fractions[item % n_fractions] * (double)all);
  need = need < 1 ? 1 : (need > all ? all : need);
  state[2 * item] = 0;
  state[2 * item + 1] = need;
  if (!all) radius_out[item] = __longlong_as_double(0x7ff8000000000000ll);
}

// one pass: per (ray slice, plane), for the fractions [first, first + count) of the tile, a ray whose key matches the
// fraction's prefix above this pass's digit adds q to the fraction's digit window
__global__ void __launch_bounds__(kEnergyBlock)
k_energy_select(int n_groups, const int64_t* __restrict__ slice_start, const int64_t* __restrict__ bucket_total,
                const int64_t* __restrict__ bucket_start, const MtfRay* __restrict__ stage, const u64* __restrict__ q,
                const u64* __restrict__ total, const double* __restrict__ centroid, const double* __restrict__ focus,
                int n_focus, int shape, int follow, int n_fractions, int first, int count, int low, int width,
                const u64* __restrict__ state, u64* __restrict__ windows) {
  __shared__ u64 window[kEnergyFractionTile][kEnergyDigits];
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int f = blockIdx.y;
  const int g = mtf_owner(slice_start, n_groups, s);
  if (g < 0 || total[g] == 0) return;
  const int digits = 1 << width;
  const size_t item = ((size_t)g * n_focus + f) * n_fractions + first;
  u64 prefix[kEnergyFractionTile];
#pragma unroll
  for (int k = 0; k < kEnergyFractionTile; ++k) {
    prefix[k] = k < count ? state[2 * (item + k)] : ~0ull;  // (no key matches all ones)
    if (k < count)
      for (int b = t; b < digits; b += kEnergyBlock) window[k][b] = 0;
  }
  __syncthreads();
  const double delta = focus[f];
  const double c1 = follow ? centroid[4 * g] + delta * centroid[4 * g + 2] : 0.0;
  const double c2 = follow ? centroid[4 * g + 1] + delta * centroid[4 * g + 3] : 0.0;
  int64_t lo, hi;
  mtf_slice(slice_start, bucket_start, bucket_total[g], g, s, lo, hi);  // (the MTF's slices)
  for (int64_t r = lo + t; r < hi; r += kEnergyBlock) {
    const u64 weight = q[r];
    if (!weight) continue;
    const u64 key = (u64)__double_as_longlong(energy_distance(stage[r], delta, c1, c2, shape));
    const u64 above = key >> (low + width);
    const int digit = (int)(key >> low) & (digits - 1);
#pragma unroll
    for (int k = 0; k < kEnergyFractionTile; ++k)
      if (above == prefix[k]) atomicAdd(&window[k][digit], weight);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kEnergyFractionTile; ++k)
    if (k < count)
      for (int b = t; b < digits; b += kEnergyBlock) {
        const u64 v = window[k][b];
        if (v) atomicAdd(windows + (item + k) * kEnergyDigits + b, v);
      }
}

// per (group, plane, fraction): the first digit where the running sum reaches the residual; the window left zeroed
__global__ void __launch_bounds__(kEnergyBlock)
k_energy_digit(int n_focus, int n_fractions, int width, int last, const u64* __restrict__ total,
               u64* __restrict__ windows, u64* __restrict__ state, double* __restrict__ radius_out) {
  __shared__ u64 scan[kEnergyBlock];
  const int t = threadIdx.x;
  const size_t item = blockIdx.x;
  if (total[item / ((size_t)n_focus * n_fractions)] == 0) return;  // (nothing was added: the window is zero)
  const int per = (1 << width) / kEnergyBlock;  // 4 or 8 tallies a thread, contiguous
  u64* const mine = windows + item * kEnergyDigits + t * per;
  // (read before the scan's barriers: the one thread that finds the digit overwrites both words after them)
  const u64 before = state[2 * item], need = state[2 * item + 1];
  u64 v[8], sum = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // (unrolled: v stays in registers)
    v[k] = k < per ? mine[k] : 0;
    if (k < per) mine[k] = 0;
    sum += v[k];
  }
  scan[t] = sum;
  __syncthreads();
  for (int off = 1; off < kEnergyBlock; off <<= 1) {
    const u64 add = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  u64 below = scan[t] - sum;
  if (below < need && need <= scan[t]) {  // (one thread: the matching rays' total is at least the residual)
    int pick = -1;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (pick < 0) {
        if (below + v[k] >= need) pick = k; else below += v[k];
      }
    const u64 prefix = (before << width) | (u64)(t * per + pick);
    state[2 * item] = prefix;
    state[2 * item + 1] = need - below;
    if (last) radius_out[item] = __longlong_as_double((long long)prefix);
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t prt_frame_energy_workspace_bytes(int64_t n_rows, int n_groups, int n_radii, int n_fractions,
                                                    int n_focus) {
  if (n_rows < 0 || n_groups < 1 || n_radii < 0 || n_radii > ENERGY_MAX_RADII || n_fractions < 0 ||
      n_fractions > ENERGY_MAX_FRACTIONS || n_radii + n_fractions < 1 || n_focus < 1 || n_focus > ENERGY_MAX_FOCUS)
    return PRT_ERR_ARG;
  if ((size_t)n_groups * n_focus * n_radii * 8 > kEnergySlabBytes ||
      (size_t)n_groups * n_focus * n_fractions * kEnergyDigits * 8 > kEnergySlabBytes)
    return PRT_ERR_ARG;  // (the two slab caps of prt_frame_energy)
  // the MTF's staging words (bucket totals and starts, chunk and slice starts, misses, centres, its record), then per
  // group pbar / sbar, w_max, shift and W, the radii, fractions and planes, the select's state, the sorted and the
  // staged rays and their integer weights
  return (4 * ((int64_t)n_groups + 1) + (1 + 3 + MTF_RECORD + 4 + 3) * (int64_t)n_groups) * 8 +
         (int64_t)(n_radii + n_fractions + n_focus) * 8 + (int64_t)n_groups * n_focus * n_fractions * 16 +
         n_rows * (int64_t)(sizeof(MtfRaw) + sizeof(MtfRay) + 8) + 64;
}

extern "C" int prt_frame_energy(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                                double generation, double rays_per_source, int n_groups, const double* reference,
                                const double* axes, int weight_column, int shape, int follow_centroid,
                                const double* radii, int n_radii, const double* fractions, int n_fractions,
                                const double* focus, int n_focus, double* energy_out, double* radius_out,
                                double* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || n_groups < 1 || !record_out || !workspace || !axes || (n_rows && !rows))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  if (shape < PRT_ENERGY_CIRCLE || shape > PRT_ENERGY_SLIT_E2)
    return fail(PRT_ERR_ARG, "energy: shape is PRT_ENERGY_CIRCLE, SQUARE, SLIT_E1 or SLIT_E2");
  if (n_radii < 0 || n_radii > ENERGY_MAX_RADII || (n_radii && (!radii || !energy_out)))
    return fail(PRT_ERR_ARG, "energy: 0 to 4096 radii, with energy_out");
  if (n_fractions < 0 || n_fractions > ENERGY_MAX_FRACTIONS || (n_fractions && (!fractions || !radius_out)))
    return fail(PRT_ERR_ARG, "energy: 0 to 16 fractions, with radius_out");
  if (n_radii + n_fractions < 1) return fail(PRT_ERR_ARG, "energy: radii or fractions, not neither");
  if (!focus || n_focus < 1 || n_focus > ENERGY_MAX_FOCUS) return fail(PRT_ERR_ARG, "energy: 1 to 256 focus shifts");
  for (int k = 0; k < n_radii; ++k)
    if (!(radii[k] >= 0 && radii[k] < PRT_INF) || (k && !(radii[k] > radii[k - 1])))
      return fail(PRT_ERR_ARG, "energy: radii finite, >= 0 and strictly ascending");
  for (int k = 0; k < n_fractions; ++k)
    if (!(fractions[k] > 0 && fractions[k] <= 1)) return fail(PRT_ERR_ARG, "energy: fractions in (0, 1]");
  for (int k = 0; k < n_focus; ++k)
    if (!std::isfinite(focus[k])) return fail(PRT_ERR_ARG, "energy: focus shifts finite");
  MtfAxes ax;
  int rc = mtf_axes(axes, ax);
  if (rc) return rc;
  if ((size_t)n_groups * n_focus * n_radii * 8 > kEnergySlabBytes)
    return fail(PRT_ERR_ARG, "energy: n_groups * n_focus * n_radii * 8 bytes above the 256 MiB slab cap");
  if ((size_t)n_groups * n_focus * n_fractions * kEnergyDigits * 8 > kEnergySlabBytes)
    return fail(PRT_ERR_ARG, "energy: n_groups * n_focus * n_fractions * 16 KiB above the 256 MiB slab cap");
  // (the slices are the MTF's with no slab to cap them: kMtfMaxSlices a group)
  const MtfRowPlan row = mtf_row_plan(n_rows, n_groups, kMtfMaxSlices);
  const int64_t chunk_grid = row.chunk_grid, slice_grid = row.slice_grid;
  if (chunk_grid > 0x7fffffff || slice_grid > 0x7fffffff)
    return fail(PRT_ERR_ARG, "energy: too many rows for one launch");
  const int planes_per_tile = n_radii ? std::max(1, std::min(n_focus, kEnergyWindow / n_radii)) : 1;
  const int plane_tiles = (n_focus + planes_per_tile - 1) / planes_per_tile;
  std::vector<double> host((size_t)n_radii + n_fractions + n_focus);
  for (int k = 0; k < n_radii; ++k) host[k] = radii[k];
  for (int k = 0; k < n_fractions; ++k) host[(size_t)n_radii + k] = fractions[k];
  for (int k = 0; k < n_focus; ++k) host[(size_t)n_radii + n_fractions + k] = focus[k];
  rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_energy_workspace_bytes)
  MtfStaging s;
  u64* w_max = (u64*)mtf_staging_words(workspace, n_groups, s);  // (missed, w_max and total are cleared together)
  u64* total = w_max + n_groups;
  int* shift = (int*)(total + n_groups);
  s.centre = (double*)(total + 2 * (size_t)n_groups);
  s.record = s.centre + 3 * (size_t)n_groups;
  double* centroid = s.record + (size_t)MTF_RECORD * n_groups;
  double* d_radii = centroid + 4 * (size_t)n_groups;
  double* d_fractions = d_radii + n_radii;
  double* planes = d_fractions + n_fractions;
  u64* state = (u64*)(planes + n_focus);
  const size_t items = (size_t)n_groups * n_focus * n_fractions;
  s.sorted = (MtfRaw*)(((uintptr_t)(state + 2 * items) + 31) & ~(uintptr_t)31);
  s.stage = (MtfRay*)(s.sorted + n_rows);
  u64* q = (u64*)(s.stage + n_rows);
  const size_t count_bytes = row.count_bytes, centre_bytes = row.centre_bytes;
  const size_t chunk_bytes = (size_t)chunk_grid * 5 * sizeof(double);
  const size_t bin_bytes = (size_t)n_groups * n_focus * n_radii * 8;
  const size_t window_bytes = items * kEnergyDigits * 8;
  char* scratch = nullptr;
  HIP_TRY(hipMallocAsync((void**)&scratch, count_bytes + centre_bytes + chunk_bytes + bin_bytes + window_bytes, st));
  s.counts = (int64_t*)scratch;
  s.centre_slab = (double*)(scratch + count_bytes);
  double* chunk_slab = (double*)(scratch + count_bytes + centre_bytes);
  u64* bins = (u64*)(scratch + count_bytes + centre_bytes + chunk_bytes);
  u64* windows = (u64*)(scratch + count_bytes + centre_bytes + chunk_bytes + bin_bytes);
  if (bin_bytes + window_bytes) HIP_TRY(hipMemsetAsync(bins, 0, bin_bytes + window_bytes, st));
  HIP_TRY(hipMemcpyAsync(d_radii, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, st));
  rc = mtf_stage_rows(st, row, s, (size_t)n_groups * 3 * 8, rows, ld, n_rows, surface, generation, rays_per_source,
                      n_groups, reference, ax, weight_column, kMtfMaxSlices);
  if (rc) return rc;
  const unsigned group_grid = (unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK);
  hipLaunchKernelGGL(k_energy_centre, dim3((unsigned)chunk_grid), dim3(kEnergyBlock), 0, st, n_groups, s.chunk_start,
                     s.bucket_total, s.bucket_start, s.stage, chunk_slab, w_max);
  hipLaunchKernelGGL(k_energy_record, dim3(group_grid), dim3(PRT_BLOCK), 0, st, n_groups, s.chunk_start, chunk_slab,
                     s.centre, s.bucket_total, s.missed, w_max, centroid, shift, record_out);
  hipLaunchKernelGGL(k_energy_scale, dim3((unsigned)chunk_grid), dim3(kEnergyBlock), 0, st, n_groups, s.chunk_start,
                     s.bucket_total, s.bucket_start, s.stage, shift, q, total);
  if (n_radii) {
    hipLaunchKernelGGL(k_energy_curve, dim3((unsigned)slice_grid, (unsigned)plane_tiles), dim3(kEnergyBlock), 0, st,
                       n_groups, s.slice_start, s.bucket_total, s.bucket_start, s.stage, q, total, centroid, planes, n_focus,
                       planes_per_tile, shape, follow_centroid ? 1 : 0, d_radii, n_radii, bins);
    hipLaunchKernelGGL(k_energy_finish, dim3((unsigned)(((int64_t)n_groups * n_focus + PRT_BLOCK - 1) / PRT_BLOCK)),
                       dim3(PRT_BLOCK), 0, st, n_groups, n_focus, n_radii, bins, total, energy_out);
  }
  if (n_fractions) {
    hipLaunchKernelGGL(k_energy_begin, dim3((unsigned)((items + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                       n_groups, n_focus, n_fractions, d_fractions, total, state, radius_out);
    for (int pass = 0; pass < kEnergyPasses; ++pass) {
      for (int first = 0; first < n_fractions; first += kEnergyFractionTile)
        hipLaunchKernelGGL(k_energy_select, dim3((unsigned)slice_grid, (unsigned)n_focus), dim3(kEnergyBlock), 0, st,
                           n_groups, s.slice_start, s.bucket_total, s.bucket_start, s.stage, q, total, centroid, planes,
                           n_focus, shape, follow_centroid ? 1 : 0, n_fractions, first,
                           std::min(kEnergyFractionTile, n_fractions - first), kEnergyLow[pass], kEnergyWidth[pass],
                           state, windows);
      hipLaunchKernelGGL(k_energy_digit, dim3((unsigned)items), dim3(kEnergyBlock), 0, st, n_focus, n_fractions,
                         kEnergyWidth[pass], pass == kEnergyPasses - 1 ? 1 : 0, total, windows, state, radius_out);
    }
  }
  return mtf_finish(st, scratch);
}

// prt_tolerance.hpp -- Monte Carlo tolerancing of the wavefront from one trace, on the device:
// the Strehl ratio of many perturbed systems under the linear ray model, OPD_r + sum_c x_rc p_c the phase of ray r, the
// merit itself not linearised; and the second moments of the OPD and its derivative columns, from which the host takes
// the RMS wavefront error of a trial and the least-squares compensators.  It stands on the Huygens core of prt_psf.hpp
// (the wavelength list, the rule for keeping a ray, the stable counting sort of prt_sort.hpp under it, the slices, the
// tree, the scratch and the status word), on prt_selection.hpp and on prt_trials.hpp.  Definitions: include/prt.h.
//
//   k_tol_rows          per selected row, in the selection's order: kept / missed / unfollowed and its (group,
//                       wavelength) bucket; per wave and bucket the rays kept; the others counted (integer atomics)
//   (k_sort_offsets, k_sort_starts of prt_sort.hpp: each wave's offset inside each bucket, each bucket's total and start)
//   k_tol_scatter       the stable counting sort of an index of the kept rays
//   k_tol_stage         per sorted ray, gathered through the index: a = sqrt(w), c0 = OPD s, e_c = x_c s, one plane each
//   k_tol_weight        per (ray slice, bucket): sum a, a fixed tree
//   k_tol_record        per group: the slices folded in order, the record and the normalisation D_g
//   k_tol_sum<CP>       per (trial tile, ray slice, bucket): a thread owns kTolTrials trials, their coefficients in
//                       registers (CP >= C of them, the rest zeros); the slice's rays go through an LDS tile and are
//                       read as broadcasts; per (ray, trial) C multiply-adds, the phase reduction of psf_phase (fract,
//                       fp32 cos and sin of the turn) and two fp64 accumulates; partial sums into a slab
//   k_tol_fold          per (group, trial): the slices added in slice order, U per wavelength and the Strehl ratio
//   k_tol_moments       per (chunk of kTolMomentChunk selected rows, group): thread e owns entry e of the lower triangle
//                       of sum w v v^T, v = (1, OPD, x_1 .. x_C), summed in row order
//   k_tol_moments_fold  per (group, entry): the chunks added in chunk order
// The slice count follows n_selected, the bucket count and the device's CU count, a slice's rays its bucket's kept count --
// never n_rows, the frame's other rows, M or C --, and a trial's arithmetic does not depend on the other trials of the
// call.  No floating-point atomics: every output is the same, bit for bit, on every run.
#pragma once

enum { TOL_MAX_COLUMNS = 20, TOL_MAX_TRIALS = 65536, TOL_RECORD = 5, TOL_BAD_WAVELENGTH = 1, TOL_BAD_ROW = 2 };
enum { TOL_KEPT = 0, TOL_MISSED = 1, TOL_UNFOLLOWED = 2, TOL_BAD = 3 };
static const int kTolBlock = 256;                     // threads of a k_tol_sum workgroup
static const int kTolTrials = 2;                      // trials a thread owns (coefficients and accumulators in registers)
static const int kTolTile = kTolBlock * kTolTrials;   // trials of a workgroup
static const int kTolRays = 128;                      // rays of the LDS tile
static const int kTolMinSlice = 2048;                 // selected rows a slice should hold at least
static const int kTolColumnStep = 4;                  // k_tol_sum is built for 4, 8, 12, 16 and 20 columns
static const int kTolMomentChunk = 2048;              // selected rows of a k_tol_moments workgroup
static const int kTolMomentRays = 64;                 // rows of its LDS tile
static_assert(kTolMinSlice == kPsfMinSlice, "psf_plan cuts the slices of every pass by kPsfMinSlice");
static_assert(1 + (TOL_MAX_COLUMNS + 1) + (TOL_MAX_COLUMNS + 1) * (TOL_MAX_COLUMNS + 2) / 2 <= kTolBlock,
              "k_tol_moments: a thread per entry");

// selected row r: its bucket, what becomes of it and its weight
struct TolRow { int bucket, state; double w; };
__device__ __forceinline__ TolRow tol_row(const double* __restrict__ rows, int64_t ld, int64_t n_rows,
                                          const int64_t* __restrict__ selected, int64_t n_selected, int64_t r,
                                          int n_groups, const int64_t* __restrict__ group_first,
                                          const double* __restrict__ opd, const double* __restrict__ columns, int C,
                                          int weight_column, const PsfLambda& lambda, int* __restrict__ status) {
  TolRow out{-1, TOL_BAD, 0.0};
  const int64_t j = selected[r];
  const int group = mtf_owner(group_first, n_groups, r);
  if (j < 0 || j >= n_rows || group < 0) {
    atomicOr(status, TOL_BAD_ROW);
    return out;
  }
  const int k = psf_wavelength(lambda, rows[PRT_COL_WAVELENGTH * ld + j]);
  if (k < 0) {
    atomicOr(status, TOL_BAD_WAVELENGTH);
    return out;
  }
  out.bucket = group * lambda.n + k;
  const double o = opd[r];
  out.w = weight_column >= 0 ? rows[(int64_t)weight_column * ld + j] : 1.0;
  if (!(psf_keep(o, 0.0, 0.0, out.w) && fabs(o) < PRT_INF)) {
    out.state = TOL_MISSED;
    return out;
  }
  bool followed = true;
  for (int c = 0; c < C; ++c) followed = followed && fabs(columns[(int64_t)c * n_selected + r]) < PRT_INF;
  out.state = followed ? TOL_KEPT : TOL_UNFOLLOWED;
  return out;
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_tol_rows(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ selected,
           int64_t n_selected, int n_groups, const int64_t* __restrict__ group_first, const double* __restrict__ opd,
           const double* __restrict__ columns, int C, int weight_column, PsfLambda lambda, int64_t per_wave,
           int* __restrict__ bucket_of, int64_t* __restrict__ counts, int buckets,
           unsigned long long* __restrict__ missed, unsigned long long* __restrict__ unfollowed,
           int* __restrict__ status) {
  const auto [lane, wave, first, last] = sort_run(per_wave, n_selected);
  if (first >= last) return;
  int64_t* const mine = counts + wave * buckets;  // (only this wave writes here)
  for (int64_t base = first; base < last; base += 64) {
    const int64_t r = base + lane;
    int bucket = -1;
    if (r < last) {
      const TolRow row = tol_row(rows, ld, n_rows, selected, n_selected, r, n_groups, group_first, opd, columns, C,
                                 weight_column, lambda, status);
      if (row.state == TOL_KEPT) bucket = row.bucket;
      else if (row.state == TOL_MISSED) atomicAdd(missed + row.bucket, 1ull);  // (integer: the same total in any order)
      else if (row.state == TOL_UNFOLLOWED) atomicAdd(unfollowed + row.bucket, 1ull);
      bucket_of[r] = bucket;
    }
    sort_tally(lane, bucket, mine);
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_tol_scatter(int64_t n_selected, int64_t per_wave, const int* __restrict__ bucket_of, int64_t* __restrict__ offsets,
              const int64_t* __restrict__ bucket_start, int buckets, int64_t* __restrict__ order) {
  const SortRun run = sort_run(per_wave, n_selected);  // (offsets + wave * buckets: only this wave reads and writes)
  psf_place(run.first, run.last, bucket_of, offsets + run.wave * buckets, bucket_start,
            [&](int64_t r, int64_t pos) { order[pos] = r; });
}

// stage: (C + 2, n_selected) planes a, c0, e_1 .. e_C of the sorted rays
__global__ void __launch_bounds__(PRT_BLOCK)
k_tol_stage(const double* __restrict__ rows, int64_t ld, const int64_t* __restrict__ selected, int64_t n_selected,
            int n_groups, const int64_t* __restrict__ group_first, int weight_column, PsfLambda lambda,
            const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start, int buckets,
            const int64_t* __restrict__ order, const double* __restrict__ opd, const double* __restrict__ columns, int C,
            double* __restrict__ stage) {
  const int64_t i = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (i >= n_selected || i >= bucket_start[buckets - 1] + bucket_total[buckets - 1]) return;
  const int64_t slot = order[i], j = selected[slot];
  const int l = psf_wavelength(lambda, rows[PRT_COL_WAVELENGTH * ld + j]);
  const double s = l < 0 ? 0.0 : lambda.s[l];
  const double w = weight_column >= 0 ? rows[(int64_t)weight_column * ld + j] : 1.0;
  stage[i] = sqrt(w);
  stage[n_selected + i] = opd[slot] * s;
  for (int c = 0; c < C; ++c) stage[(int64_t)(2 + c) * n_selected + i] = columns[(int64_t)c * n_selected + slot] * s;
}

// weight_slab: (bucket, slice), sum a
__global__ void __launch_bounds__(kPsfBlock)
k_tol_weight(const double* __restrict__ stage, const int64_t* __restrict__ bucket_total,
             const int64_t* __restrict__ bucket_start, int slices, double* __restrict__ weight_slab) {
  __shared__ double red[1][kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.x, b = blockIdx.y;
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, b, slice, slices, lo, hi);
  double sum = 0.0;
  for (int64_t r = lo + t; r < hi; r += kPsfBlock) sum += stage[r];
  red[0][t] = sum;
  sort_tree(red, t);
  if (t == 0) weight_slab[(size_t)b * slices + slice] = red[0][0];
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_tol_record(const double* __restrict__ weight_slab, int slices, int n_groups, PsfLambda lambda,
             const int64_t* __restrict__ bucket_total, const unsigned long long* __restrict__ missed,
             const unsigned long long* __restrict__ unfollowed, double* __restrict__ record_out,
             double* __restrict__ norm) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  double denominator = 0.0;
  for (int l = 0; l < lambda.n; ++l) {
    const int b = g * lambda.n + l;
    double a = 0.0;
    for (int q = 0; q < slices; ++q) a += weight_slab[(size_t)b * slices + q];
    const double inv = lambda.s[l], den = (inv * a) * (inv * a);
    double* o = record_out + (size_t)b * TOL_RECORD;
    o[0] = (double)bucket_total[b];
    o[1] = (double)missed[b];
    o[2] = (double)unfollowed[b];
    o[3] = a;
    o[4] = den;
    denominator += den;
  }
  norm[g] = denominator;
}

// Thread t owns the trials first + blockIdx.x * kTolTile + t * kTolTrials + q of group g, q < kTolTrials, and of each
// its C coefficients p (those from C to CP are zeros, and so are the tile's e there: fma(0, 0, phi) is phi).
// phi = fma(e_C, p_C, ... fma(e_1, p_1, c0)), the columns in their order.
// trials: (n_groups, M, C); slab: (bucket, slice, n_trials, 2), the sums of a (cos, sin) of this launch's trials
template <int CP>
__global__ void __launch_bounds__(kTolBlock)
k_tol_sum(const double* __restrict__ stage, int64_t n_items, const int64_t* __restrict__ bucket_total,
          const int64_t* __restrict__ bucket_start, const double* __restrict__ trials, int n_lambda, int M, int C,
          int first, int n_trials, int slices, double* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) double tile[kTolRays][CP + 2];
  const int t = threadIdx.x, slice = blockIdx.y, b = blockIdx.z, g = b / n_lambda;
  const int mine = (int)blockIdx.x * kTolTile + t * kTolTrials;  // (the first of this thread's trials, in the launch)
  const bool busy = (int)blockIdx.x * kTolTile + (t & ~63) * kTolTrials < n_trials;  // (the same in a wave's lanes)
  double p[kTolTrials][CP], re[kTolTrials], im[kTolTrials];
#pragma unroll
  for (int q = 0; q < kTolTrials; ++q) {
    const bool valid = mine + q < n_trials;
    const double* from = trials + ((int64_t)g * M + (valid ? first + mine + q : 0)) * C;
#pragma unroll
    for (int c = 0; c < CP; ++c) p[q][c] = valid && c < C ? from[c] : 0.0;
    re[q] = im[q] = 0.0;
  }
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, b, slice, slices, lo, hi);
  for (int64_t base = lo; base < hi; base += kTolRays) {
    const int count = hi - base < kTolRays ? (int)(hi - base) : kTolRays;
    __syncthreads();  // (the previous tile is read)
    for (int i = t; i < kTolRays * (CP + 2); i += kTolBlock) {
      const int v = i / kTolRays, ray = i - v * kTolRays;  // (a wave reads 64 rays of one plane)
      tile[ray][v] = ray < count && v < C + 2 ? stage[(int64_t)v * n_items + base + ray] : 0.0;
    }
    __syncthreads();
    if (busy) {
      for (int r = 0; r < count; ++r) {
        const double* __restrict__ ray = tile[r];
        const double a = ray[0], c0 = ray[1];
#pragma unroll
        for (int q = 0; q < kTolTrials; ++q) {
          double phase = c0;
#pragma unroll
          for (int c = 0; c < CP; ++c) phase = fma(ray[2 + c], p[q][c], phase);
          const float turn = (float)__builtin_amdgcn_fract(phase);  // [0, 1), as psf_phase reduces it
          re[q] = fma(a, (double)__builtin_amdgcn_cosf(turn), re[q]);
          im[q] = fma(a, (double)__builtin_amdgcn_sinf(turn), im[q]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kTolTrials; ++q)
    if (mine + q < n_trials) {
      double* o = slab + (((size_t)b * slices + slice) * n_trials + mine + q) * 2;
      o[0] = re[q];
      o[1] = im[q];
    }
}

// U_glm = s (sum a cos, sum a sin); Strehl_gm = sum_l s^2 (C^2 + S^2) / D_g, as k_psfg_record forms it
__global__ void __launch_bounds__(PRT_BLOCK)
k_tol_fold(const double* __restrict__ slab, int slices, int n_groups, int M, int first, int n_trials, PsfLambda lambda,
           const double* __restrict__ norm, double* __restrict__ strehl_out, double* __restrict__ amplitude_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * n_trials) return;
  const int g = (int)(item / n_trials), m = (int)(item - (int64_t)g * n_trials);
  const double d = norm[g], nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool lit = d > 0.0;  // (a group without kept rays, or without weight: NaN)
  double numerator = 0.0;
  for (int l = 0; l < lambda.n; ++l) {
    const int b = g * lambda.n + l;
    double re = 0.0, im = 0.0;
    for (int q = 0; q < slices; ++q) {
      const double* p = slab + (((size_t)b * slices + q) * n_trials + m) * 2;
      re += p[0];
      im += p[1];
    }
    const double inv = lambda.s[l];
    double* o = amplitude_out + ((size_t)b * M + first + m) * 2;
    o[0] = lit ? inv * re : nan;
    o[1] = lit ? inv * im : nan;
    numerator += inv * inv * (re * re + im * im);
  }
  strehl_out[(size_t)g * M + first + m] = lit ? numerator / d : nan;
}

// the place of entry e in v v^T, v = (1, y_0 .. y_C): the lower triangle by rows
__device__ __forceinline__ void tol_entry(int e, int& l, int& r) {
  l = 0;
  while ((l + 1) * (l + 2) / 2 <= e) ++l;
  r = e - l * (l + 1) / 2;
}

// workgroup (chunk, group): the rows [group_first[group] + chunk * kTolMomentChunk, ...) of the group; its sums to
// partials[(chunk_first[group] + chunk) * entries + e]; counters: (n_groups, 3) rays kept, missed, unfollowed
__global__ void __launch_bounds__(kTolBlock)
k_tol_moments(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ selected,
              int64_t n_selected, int n_groups, const int64_t* __restrict__ group_first,
              const int64_t* __restrict__ chunk_first, const double* __restrict__ opd,
              const double* __restrict__ columns, int C, int weight_column, PsfLambda lambda,
              double* __restrict__ partials, unsigned long long* __restrict__ counters, int* __restrict__ status) {
  __shared__ double tile[kTolMomentRays][TOL_MAX_COLUMNS + 3];  // w, then v
  const int group = blockIdx.y, t = threadIdx.x, entries = (C + 2) * (C + 3) / 2;
  if ((int64_t)blockIdx.x >= chunk_first[group + 1] - chunk_first[group]) return;  // (the whole workgroup)
  const int64_t begin = group_first[group] + (int64_t)blockIdx.x * kTolMomentChunk;
  const int64_t end = begin + kTolMomentChunk < group_first[group + 1] ? begin + kTolMomentChunk : group_first[group + 1];
  int el = 0, er = 0;
  if (t < entries) tol_entry(t, el, er);
  double acc = 0.0;
  int tally[3] = {0, 0, 0};  // (the first wave's: rows kept, missed, unfollowed of this chunk, the same in every lane)
  for (int64_t base = begin; base < end; base += kTolMomentRays) {
    const int here = end - base < kTolMomentRays ? (int)(end - base) : kTolMomentRays;
    __syncthreads();  // (the previous tile is read)
    int state = TOL_BAD;
    if (t < here) {
      const int64_t r = base + t;
      const TolRow row = tol_row(rows, ld, n_rows, selected, n_selected, r, n_groups, group_first, opd, columns, C,
                                 weight_column, lambda, status);
      const bool live = row.state == TOL_KEPT;
      state = row.state;
      double* v = tile[t];
      v[0] = live ? row.w : 0.0;
      v[1] = live ? 1.0 : 0.0;
      v[2] = live ? opd[r] : 0.0;
      for (int c = 0; c < C; ++c) v[3 + c] = live ? columns[(int64_t)c * n_selected + r] : 0.0;
    }
    if (t < 64) {  // (the tile's rows are the first wave's lanes: a ballot per state, no atomic per row)
#pragma unroll
      for (int q = 0; q < 3; ++q) tally[q] += __popcll(__ballot(state == q));
    }
    __syncthreads();
    if (t < entries)
      for (int k = 0; k < here; ++k) acc = fma(tile[k][0] * tile[k][1 + el], tile[k][1 + er], acc);
  }
  if (t < entries) partials[(chunk_first[group] + blockIdx.x) * entries + t] = acc;
  if (t < 3 && tally[t]) atomicAdd(counters + (size_t)group * 3 + t, (unsigned long long)tally[t]);  // (integer, one a chunk)
}

// moments_out: (n_groups, 3 + entries): rays kept, n_missed, n_unfollowed, sum w, sum w y_i (C + 1), then
// sum w y_i y_j, j <= i, by rows
__global__ void __launch_bounds__(PRT_BLOCK)
k_tol_moments_fold(const double* __restrict__ partials, const int64_t* __restrict__ chunk_first, int n_groups, int C,
                   const unsigned long long* __restrict__ counters, double* __restrict__ moments_out) {
  const int entries = (C + 2) * (C + 3) / 2, width = 3 + entries;
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * width) return;
  const int g = (int)(item / width), o = (int)(item - (int64_t)g * width);
  if (o < 3) {
    moments_out[item] = (double)counters[(size_t)g * 3 + o];
    return;
  }
  // output entry o - 3: sum w (0, 0); sum w y_i (i + 1, 0); sum w y_i y_j (i + 1, j + 1)
  int l = 0, r = 0, e = o - 3;
  if (e >= 1 && e < C + 2) {
    l = e;
  } else if (e >= C + 2) {
    tol_entry(e - (C + 2), l, r);
    ++l;
    ++r;
  }
  const int at = l * (l + 1) / 2 + r;
  double sum = 0.0;
  for (int64_t c = chunk_first[g]; c < chunk_first[g + 1]; ++c) sum += partials[c * entries + at];
  moments_out[item] = sum;
}

// ---- entry points ---------------------------------------------------------------------------------------------------
// what both entries check before a device is touched
static int tol_arguments(const char* name, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                         int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                         const double* opd, const double* columns, int n_columns, const double* wavelengths_um,
                         int n_wavelengths, double world_unit_um, PsfLambda& lambda) {
  const std::string at = std::string(name) + ": ";
  if (n_rows < 0 || ld < n_rows || n_selected < 0 || n_groups < 1 || !group_first || !wavelengths_um || (n_rows && !rows))
    return fail(PRT_ERR_ARG, at + "bad buffers");
  if (n_columns < 1 || n_columns > TOL_MAX_COLUMNS) return fail(PRT_ERR_ARG, at + "1 to 20 columns");
  if (n_selected && (!selected || !opd || !columns))
    return fail(PRT_ERR_ARG, at + "selected, opd and columns where rows are selected");
  int rc = selection_check(name, n_rows, n_selected, group_first, n_groups, weight_column);
  if (!rc) rc = psf_lambda(name, wavelengths_um, n_wavelengths, world_unit_um, lambda);
  if (rc) return rc;
  if ((int64_t)n_groups * n_wavelengths > 16383) return fail(PRT_ERR_ARG, at + "n_groups * n_wavelengths <= 16383");
  return PRT_OK;
}

static int64_t tol_moment_chunks(int64_t n_selected, int n_groups) {
  return n_selected / kTolMomentChunk + n_groups;  // (at least the sum of the groups' chunks)
}

extern "C" int64_t prt_frame_tolerance_moments_workspace_bytes(int64_t n_selected, int n_groups, int n_columns,
                                                               int n_wavelengths) {
  if (n_selected < 0 || n_groups < 1 || n_columns < 1 || n_columns > TOL_MAX_COLUMNS || n_wavelengths < 1 ||
      n_wavelengths > PSF_MAX_WAVELENGTHS || (int64_t)n_groups * n_wavelengths > 16383)
    return PRT_ERR_ARG;
  // group starts, chunk starts, the counters, the status word, the chunks' partial sums
  return 2 * ((int64_t)n_groups + 1) * 8 + (int64_t)n_groups * 3 * 8 + 8 +
         tol_moment_chunks(n_selected, n_groups) * ((n_columns + 2) * (n_columns + 3) / 2) * 8 + 64;
}

extern "C" int prt_frame_tolerance_moments(int device, const double* rows, int64_t ld, int64_t n_rows,
                                           const int64_t* selected, int64_t n_selected, const int64_t* group_first,
                                           int n_groups, int weight_column, const double* opd, const double* columns,
                                           int n_columns, const double* wavelengths_um, int n_wavelengths,
                                           double world_unit_um, double* moments_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  const int C = n_columns;
  if (!moments_out || !workspace) return fail(PRT_ERR_ARG, "tolerance_moments: bad buffers");
  PsfLambda lambda;
  int rc = tol_arguments("tolerance_moments", rows, ld, n_rows, selected, n_selected, group_first, n_groups,
                         weight_column, opd, columns, C, wavelengths_um, n_wavelengths, world_unit_um, lambda);
  if (rc) return rc;
  std::vector<int64_t> chunk_first((size_t)n_groups + 1, 0);
  int64_t most = 1;
  for (int g = 0; g < n_groups; ++g) {
    const int64_t chunks = (group_first[g + 1] - group_first[g] + kTolMomentChunk - 1) / kTolMomentChunk;
    chunk_first[g + 1] = chunk_first[g] + chunks;
    most = std::max(most, chunks);
  }
  const int entries = (C + 2) * (C + 3) / 2;
  if (most > 0x7fffffff || n_groups > 65535 || ((int64_t)n_groups * (3 + entries) + PRT_BLOCK - 1) / PRT_BLOCK > 0x7fffffff)
    return fail(PRT_ERR_ARG, "tolerance_moments: too many rows or groups for one launch");
  rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_tolerance_moments_workspace_bytes)
  int64_t* d_group = (int64_t*)workspace;
  int64_t* d_chunk = d_group + (n_groups + 1);
  unsigned long long* counters = (unsigned long long*)(d_chunk + (n_groups + 1));
  int* status = (int*)(counters + 3 * (size_t)n_groups);
  double* partials = (double*)(status + 2);
  HIP_TRY(hipMemsetAsync(counters, 0, (size_t)n_groups * 3 * 8 + 8, st));  // (the counters and the status word)
  HIP_TRY(hipMemcpyAsync(d_group, group_first, ((size_t)n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_chunk, chunk_first.data(), ((size_t)n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_tol_moments, dim3((unsigned)most, (unsigned)n_groups), dim3(kTolBlock), 0, st, rows, ld, n_rows,
                     selected, n_selected, n_groups, d_group, d_chunk, opd, columns, C, weight_column, lambda, partials,
                     counters, status);
  hipLaunchKernelGGL(k_tol_moments_fold, dim3((unsigned)(((int64_t)n_groups * (3 + entries) + PRT_BLOCK - 1) / PRT_BLOCK)),
                     dim3(PRT_BLOCK), 0, st, partials, d_chunk, n_groups, C, counters, moments_out);
  int host_status = 0;
  HIP_TRY(hipMemcpyAsync(&host_status, status, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the host arrays outlive their copies)
  HIP_TRY(hipGetLastError());
  if (host_status & TOL_BAD_ROW) return fail(PRT_ERR_ARG, "tolerance_moments: a selected row number is outside the frame");
  if (host_status & TOL_BAD_WAVELENGTH)
    return fail(PRT_ERR_ARG, "tolerance_moments: a selected row's wavelength is not in the list");
  return PRT_OK;
}

extern "C" int64_t prt_frame_tolerance_workspace_bytes(int64_t n_selected, int n_groups, int n_columns,
                                                       int n_wavelengths, int n_trials) {
  if (n_selected < 0 || n_groups < 1 || n_columns < 1 || n_columns > TOL_MAX_COLUMNS || n_wavelengths < 1 ||
      n_wavelengths > PSF_MAX_WAVELENGTHS || (int64_t)n_groups * n_wavelengths > 16383 || n_trials < 1 ||
      n_trials > TOL_MAX_TRIALS)
    return PRT_ERR_ARG;
  // group starts, bucket totals / starts / missed / unfollowed, the status word, the groups' normalisation, the staged
  // planes, the sort's index, the rays' buckets
  return ((int64_t)n_groups + 1) * 8 + 4 * psf_buckets_bytes(n_groups, n_wavelengths) + 8 + (int64_t)n_groups * 8 +
         n_selected * (int64_t)((n_columns + 2) * sizeof(double) + sizeof(int64_t) + sizeof(int)) + 64;
}

extern "C" int prt_frame_tolerance(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                                   int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                                   const double* opd, const double* columns, int n_columns,
                                   const double* wavelengths_um, int n_wavelengths, double world_unit_um,
                                   const double* trials, int n_trials, double* strehl_out, double* amplitude_out,
                                   double* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  const int C = n_columns, M = n_trials;
  if (!trials || !strehl_out || !amplitude_out || !record_out || !workspace)
    return fail(PRT_ERR_ARG, "tolerance: bad buffers");
  if (M < 1 || M > TOL_MAX_TRIALS) return fail(PRT_ERR_ARG, "tolerance: 1 to 65536 trials");
  PsfLambda lambda;
  int rc = tol_arguments("tolerance", rows, ld, n_rows, selected, n_selected, group_first, n_groups, weight_column, opd,
                         columns, C, wavelengths_um, n_wavelengths, world_unit_um, lambda);
  if (rc) return rc;
  const int64_t buckets = (int64_t)n_groups * n_wavelengths;
  int cus = 1;
  rc = psf_device(device, &cus);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_tolerance_workspace_bytes)
  int64_t* d_group = (int64_t*)workspace;
  int64_t* bucket_total = d_group + (n_groups + 1);
  int64_t* bucket_start = bucket_total + buckets;
  unsigned long long* missed = (unsigned long long*)(bucket_start + buckets);
  unsigned long long* unfollowed = missed + buckets;
  int* status = (int*)(unfollowed + buckets);
  double* norm = (double*)(status + 2);
  double* stage = (double*)(((uintptr_t)(norm + n_groups) + 31) & ~(uintptr_t)31);
  int64_t* order = (int64_t*)(stage + (size_t)(C + 2) * n_selected);
  int* bucket_of = (int*)(order + n_selected);
  // the slices: one "pixel", so that they follow the selection's size, the buckets and the CUs and nothing else; the
  // slab holds the trials of one launch, at most `chunk` of them, whole tiles under the cap
  PsfPlan plan = psf_plan(cus, n_selected, buckets, buckets, 1, 1, 16, 0, 1);
  const int slices = (int)plan.slices;
  int64_t chunk = (int64_t)(kPsfSlabBytes / ((size_t)buckets * slices * 16)) / kTolTile * kTolTile;
  chunk = std::min<int64_t>(chunk, ((int64_t)M + kTolTile - 1) / kTolTile * kTolTile);
  if (chunk < kTolTile || (n_selected + PRT_BLOCK - 1) / PRT_BLOCK > 0x7fffffff)
    return fail(PRT_ERR_ARG, "tolerance: too many rows or buckets for one launch");
  plan.slab_bytes = (size_t)buckets * slices * std::min<int64_t>(chunk, M) * 16;
  PsfScratch scratch;
  rc = psf_scratch(st, plan, missed, (size_t)buckets * 16 + 8, scratch);  // (missed, unfollowed and the status word)
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(d_group, group_first, ((size_t)n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_tol_rows, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, selected, n_selected,
                     n_groups, d_group, opd, columns, C, weight_column, lambda, plan.per_wave, bucket_of, scratch.counts,
                     (int)buckets, missed, unfollowed, status);
  sort_offsets(st, (int)plan.all_waves, (int)buckets, scratch.counts, bucket_total, bucket_start);
  hipLaunchKernelGGL(k_tol_scatter, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, n_selected, plan.per_wave, bucket_of,
                     scratch.counts, bucket_start, (int)buckets, order);
  if (n_selected)
    hipLaunchKernelGGL(k_tol_stage, dim3((unsigned)((n_selected + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                       rows, ld, selected, n_selected, n_groups, d_group, weight_column, lambda, bucket_total,
                       bucket_start, (int)buckets, order, opd, columns, C, stage);
  hipLaunchKernelGGL(k_tol_weight, dim3((unsigned)slices, (unsigned)buckets), dim3(kPsfBlock), 0, st, stage,
                     bucket_total, bucket_start, slices, scratch.strehl_slab);
  hipLaunchKernelGGL(k_tol_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     scratch.strehl_slab, slices, n_groups, lambda, bucket_total, missed, unfollowed, record_out, norm);
  // the smallest instantiation that holds the columns; the trials in launches of at most `chunk`
  auto sum = [&](auto held, int first, int n) {
    hipLaunchKernelGGL(k_tol_sum<decltype(held)::value>,
                       dim3((unsigned)((n + kTolTile - 1) / kTolTile), (unsigned)slices, (unsigned)buckets),
                       dim3(kTolBlock), 0, st, stage, n_selected, bucket_total, bucket_start, trials, n_wavelengths, M, C,
                       first, n, slices, scratch.slab);
  };
  trial_launches(M, chunk, [&](int first, int n) {
    trial_columns<TOL_MAX_COLUMNS>(C, sum, first, n);
    hipLaunchKernelGGL(k_tol_fold, dim3((unsigned)(((int64_t)n_groups * n + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK),
                       0, st, scratch.slab, slices, n_groups, M, first, n, lambda, norm, strehl_out, amplitude_out);
  });
  int host_status;
  rc = psf_finish(st, status, scratch, &host_status);
  if (rc) return rc;
  if (host_status & TOL_BAD_ROW) return fail(PRT_ERR_ARG, "tolerance: a selected row number is outside the frame");
  if (host_status & TOL_BAD_WAVELENGTH)
    return fail(PRT_ERR_ARG, "tolerance: a selected row's wavelength is not in the list");
  return PRT_OK;
}

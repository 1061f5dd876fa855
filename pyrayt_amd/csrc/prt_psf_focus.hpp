// prt_psf_focus.hpp -- the diffraction PSF and the Strehl ratio through focus, on the device.
// It stands on the Huygens core of prt_psf.hpp: psf_lambda, psf_grid, psf_plan, the count, scan, offsets and place
// pieces, psf_sqrt, psf_chief_phase, the folds, and prt_sort.hpp's tree.  Definitions: include/prt.h.
//
// A pixel of plane delta lies at x = P + u e1 + v e2 + delta a, and a ray's point on the reference sphere at
// E = P + p1 e1 + p2 e2 + p3 a, so |x - E|^2 = R^2 + u^2 + v^2 + delta^2 - 2 (u p1 + v p2 + delta p3): the sum of
// prt_frame_psf with one more term.  p3 is not kept by the wavefront pass, and its sign follows the ray's direction,
// so the staging pass extends the row to the sphere again.
//
//   k_psf_count, k_psf_strehl, k_psf_record and the scans of prt_sort.hpp, as prt_frame_psf launches them
//   k_psff_stage      k_psf_stage, and p3 = (E - P).a of the row extended to the sphere (axial_out, in the wavefront's order)
//   k_psff_scatter    the stable counting sort, p3 moved beside its PsfRay into an array of its own
//   k_psff_line       per (ray slice, bucket): sum w p1, w p2, w p3, a fixed tree
//   k_psff_line_fold  per group: the slices in slice order, then the buckets in bucket order; the chief line's slopes
//   k_psff_centres    per (group, plane): the grid's centre fma(delta, t, u0)
//   k_psff_strehl     per (ray slice, bucket, plane): k_psf_strehl's sum with the chief phase at the line's point of the plane
//   k_psff_strehl_fold  per (group, plane): k_psf_record's ratio over the same denominator
//   k_psff_huygens    k_psf_huygens with a plane index: per (pixel tile, ray slice, (bucket, plane))
//   k_psff_fold       per (bucket, plane, pixel): the slices added in slice order, |U|^2 / lambda_w^2, normalised
// The ray slices are those prt_frame_psf picks for one plane's grid; planes never change them.  Planes that do not fit
// the slab cap go through it in chunks, launch after launch.  No floating-point atomics.
#pragma once

enum { PSFF_MAX_PLANES = 256 };

// the phase path of prt_psf.hpp's psf_phase with the axial term innermost: with mw = -0.0 (delta = 0) the innermost
// fma returns k0 itself, and the expression is psf_phase's
__device__ __forceinline__ PsfPhase psff_phase(double mu, double mv, double mw, double k0, double p1, double p2,
                                               double p3, double c, double s) {
  PsfPhase out;
  const double d2 = fma(mu, p1, fma(mv, p2, fma(mw, p3, k0)));  // |x - E|^2
  const double phase = fma(psf_sqrt(d2, out.inverse), s, c);    // (OPD + d - R) / lambda_w, cycles
  const float turn = (float)__builtin_amdgcn_fract(phase);      // [0, 1)
  out.cs = (double)__builtin_amdgcn_cosf(turn);
  out.sn = (double)__builtin_amdgcn_sinf(turn);
  return out;
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_psff_stage(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface, double generation,
             double rays_per_source, int n_groups, int64_t per_wave, const int64_t* __restrict__ wave_offset,
             const double* __restrict__ opd, const double* __restrict__ pupil, const double* __restrict__ group_record,
             int weight_column, PsfLambda lambda, WfAxes axes, PsfRay* __restrict__ stage, double* __restrict__ axial,
             int* __restrict__ bucket_of, int64_t* __restrict__ counts, int buckets,
             unsigned long long* __restrict__ skipped, int* __restrict__ status) {
  const auto [lane, wave, first, last] = sort_run(per_wave, n_rows);
  if (first >= last) return;
  int64_t* const mine = counts + wave * buckets;  // (only this wave writes here)
  int64_t at = wave_offset[wave];
  for (int64_t base = first; base < last; base += 64) {
    const int64_t j = base + lane;
    int group = -1;
    const bool chosen = j < last && psf_row(rows, ld, j, surface, generation, rays_per_source, n_groups, group);
    const unsigned long long ballot = __ballot(chosen);
    int bucket = -1;
    if (chosen) {
      const int64_t pos = at + __popcll(ballot & ((1ull << lane) - 1ull));
      const double* g = group_record + (size_t)group * WF_GROUP;
      const double o = opd[pos], x = pupil[2 * pos], y = pupil[2 * pos + 1];
      // the row extended to the sphere, as the wavefront pass did it: the same E, and the component it did not keep
      double p3 = __longlong_as_double(0x7ff8000000000000ll), reach, e[3];
      if (x == x && y == y && wf_extend(rows, ld, j, g, g[3], reach, e)) {
        const double v[3] = {e[0] - g[0], e[1] - g[1], e[2] - g[2]};
        p3 = v[0] * axes.a[0] + v[1] * axes.a[1] + v[2] * axes.a[2];
      }
      axial[pos] = p3;
      const int k = psf_wavelength(lambda, rows[PRT_COL_WAVELENGTH * ld + j]);
      if (k < 0) {
        atomicOr(status, PSF_BAD_WAVELENGTH);
      } else {
        const double w = weight_column >= 0 ? rows[(int64_t)weight_column * ld + j] : 1.0;
        if (psf_keep(o, x, y, w) && fabs(p3) < PRT_INF) {
          bucket = group * lambda.n + k;
          const double rho = g[5], s = lambda.s[k];
          stage[pos] = PsfRay{x * rho, y * rho, (o - g[3]) * s, sqrt(w)};
        } else {
          atomicAdd(skipped + group * lambda.n + k, 1ull);  // (integer: the same total in any order)
        }
      }
      bucket_of[pos] = bucket;
    }
    at += __popcll(ballot);
    sort_tally(lane, bucket, mine);
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_psff_scatter(const int64_t* __restrict__ wave_rows, const int64_t* __restrict__ wave_offset,
               const int* __restrict__ bucket_of, const PsfRay* __restrict__ stage, const double* __restrict__ axial,
               int64_t* __restrict__ offsets, const int64_t* __restrict__ bucket_start, int buckets,
               PsfRay* __restrict__ sorted, double* __restrict__ sorted3) {
  const int64_t wave = sort_wave();
  const int64_t from = wave_offset[wave];  // (offsets + wave * buckets: only this wave reads and writes there)
  psf_place(from, from + wave_rows[wave], bucket_of, offsets + wave * buckets, bucket_start, [&](int64_t r, int64_t pos) {
    sorted[pos] = stage[r];
    sorted3[pos] = axial[r];
  });
}

// line_slab: (bucket, slice, 3) = sum w p1, sum w p2, sum w p3 of the slice's rays, w = a^2
__global__ void __launch_bounds__(kPsfBlock)
k_psff_line(const PsfRay* __restrict__ sorted, const double* __restrict__ sorted3,
            const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start, int slices,
            double* __restrict__ line_slab) {
  __shared__ double red[3][kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.x, b = blockIdx.y;
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, b, slice, slices, lo, hi);
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int64_t r = lo + t; r < hi; r += kPsfBlock) {
    const PsfRay ray = sorted[r];
    const double w = ray.a * ray.a;
    s1 += w * ray.p1;
    s2 += w * ray.p2;
    s3 += w * sorted3[r];
  }
  red[0][t] = s1; red[1][t] = s2; red[2][t] = s3;
  sort_tree(red, t);
  if (t < 3) line_slab[((size_t)b * slices + slice) * 3 + t] = red[t][0];
}

// the chief line of a group goes through P along the weighted mean of its rays' sphere points: per unit of delta it
// moves by t_i = (sum w p_i) / (sum w p3), the slope (u.e_i) / (u.a) of a ray that runs from E to P.  track 0: 0
__global__ void __launch_bounds__(PRT_BLOCK)
k_psff_line_fold(const double* __restrict__ line_slab, int slices, int n_groups, int n_lambda, int track,
                 double* __restrict__ line_out) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  double sum[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < n_lambda; ++k) {
    const int b = g * n_lambda + k;
    double mine[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < slices; ++q)
      for (int i = 0; i < 3; ++i) mine[i] += line_slab[((size_t)b * slices + q) * 3 + i];
    for (int i = 0; i < 3; ++i) sum[i] += mine[i];
  }
  line_out[2 * g] = track ? sum[0] / sum[2] : 0.0;  // (a group without rays: 0 / 0, NaN)
  line_out[2 * g + 1] = track ? sum[1] / sum[2] : 0.0;
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_psff_centres(const double* __restrict__ line, const double* __restrict__ focus, int n_groups, int n_focus, double u0,
               double v0, double* __restrict__ centres_out) {
  const int item = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= n_groups * n_focus) return;
  const int g = item / n_focus, f = item - g * n_focus;
  centres_out[2 * item] = fma(focus[f], line[2 * g], u0);
  centres_out[2 * item + 1] = fma(focus[f], line[2 * g + 1], v0);
}

// plane_slab: (bucket, slice, plane, 2) = sum a cos, sum a sin of the phase at x_f = P + delta_f (t1 e1 + t2 e2 + a).
// d = sqrt(|x_f - E|^2) correctly rounded: at delta = 0 it is sqrt(fl(R^2)) = R, and the sum is k_psf_strehl's
__global__ void __launch_bounds__(kPsfBlock)
k_psff_strehl(const PsfRay* __restrict__ sorted, const double* __restrict__ sorted3,
              const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
              const double* __restrict__ groups, const double* __restrict__ line, const double* __restrict__ focus,
              PsfLambda lambda, int slices, int n_focus, double* __restrict__ plane_slab) {
  __shared__ double red[2][kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.x, b = blockIdx.y, f = blockIdx.z;
  const int g = b / lambda.n;
  const double s = lambda.s[b - g * lambda.n], radius = groups[(size_t)g * WF_GROUP + 3];
  const double delta = focus[f], u = delta * line[2 * g], v = delta * line[2 * g + 1];
  const double mu = -2.0 * u, mv = -2.0 * v, mw = -2.0 * delta;
  const double k0 = radius * radius + u * u + v * v + delta * delta;
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, b, slice, slices, lo, hi);
  double sum_c = 0.0, sum_s = 0.0;
  for (int64_t r = lo + t; r < hi; r += kPsfBlock) {
    const PsfRay ray = sorted[r];
    const double d = sqrt(fma(mu, ray.p1, fma(mv, ray.p2, fma(mw, sorted3[r], k0))));
    double sn, cs;
    psf_chief_phase(d, s, ray.c, sn, cs);
    sum_c += ray.a * cs;
    sum_s += ray.a * sn;
  }
  red[0][t] = sum_c; red[1][t] = sum_s;
  sort_tree(red, t);
  if (t < 2) plane_slab[((((size_t)b * slices + slice) * n_focus) + f) * 2 + t] = red[t][0];
}

// k_psf_record's ratio per (group, plane): the slices in slice order, the buckets in bucket order, over norm[g]
__global__ void __launch_bounds__(PRT_BLOCK)
k_psff_strehl_fold(const double* __restrict__ plane_slab, int slices, int n_groups, int n_focus, PsfLambda lambda,
                   const double* __restrict__ norm, double* __restrict__ strehl_out) {
  const int item = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= n_groups * n_focus) return;
  const int g = item / n_focus, f = item - g * n_focus;
  double numerator = 0.0;
  for (int k = 0; k < lambda.n; ++k) {
    const int b = g * lambda.n + k;
    double c = 0.0, s = 0.0;
    for (int q = 0; q < slices; ++q) {
      const double* p = plane_slab + ((((size_t)b * slices + q) * n_focus) + f) * 2;
      c += p[0]; s += p[1];
    }
    const double inv = lambda.s[k], num = inv * inv * (c * c + s * s);
    numerator += num;
  }
  const double denominator = norm[g];
  strehl_out[item] = denominator > 0.0 ? numerator / denominator : __longlong_as_double(0x7ff8000000000000ll);
}

// blockIdx.z = bucket * planes + plane of the chunk [first, first + planes).  slab: (bucket, plane, slice, pixel, 2)
__global__ void __launch_bounds__(kPsfBlock)
k_psff_huygens(const PsfRay* __restrict__ sorted, const double* __restrict__ sorted3,
               const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
               const double* __restrict__ group_record, const double* __restrict__ focus,
               const double* __restrict__ centres, PsfLambda lambda, int nx, int ny, double du, double dv, int slices,
               int n_focus, int first, int planes, double* __restrict__ slab) {
  __shared__ PsfRay tile[kPsfBlock];
  __shared__ double tile3[kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.y, b = blockIdx.z / planes, f = blockIdx.z - b * planes;
  const int g = b / lambda.n;
  const double s = lambda.s[b - g * lambda.n], radius = group_record[(size_t)g * WF_GROUP + 3];
  const double delta = focus[first + f], mw = -2.0 * delta;
  const double u0 = centres[2 * ((size_t)g * n_focus + first + f)], v0 = centres[2 * ((size_t)g * n_focus + first + f) + 1];
  const int64_t npix = (int64_t)nx * ny;
  double mu[kPsfPix], mv[kPsfPix], k0[kPsfPix], re[kPsfPix], im[kPsfPix];
#pragma unroll
  for (int q = 0; q < kPsfPix; ++q) {
    double u, v;
    psf_pixel((int64_t)blockIdx.x * kPsfTile + q * kPsfBlock + t, npix, nx, ny, du, dv, u0, v0, u, v);
    mu[q] = -2.0 * u;
    mv[q] = -2.0 * v;
    k0[q] = radius * radius + u * u + v * v + delta * delta;
    re[q] = im[q] = 0.0;
  }
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, b, slice, slices, lo, hi);
  for (int64_t base = lo; base < hi; base += kPsfBlock) {
    __syncthreads();  // (the previous tile is read)
    if (base + t < hi) {
      tile[t] = sorted[base + t];
      tile3[t] = sorted3[base + t];
    }
    __syncthreads();
    const int count = hi - base < kPsfBlock ? (int)(hi - base) : kPsfBlock;
    for (int r = 0; r < count; ++r) {
      const PsfRay ray = tile[r];
      const double p3 = tile3[r];
#pragma unroll
      for (int q = 0; q < kPsfPix; ++q) {
        const PsfPhase at = psff_phase(mu[q], mv[q], mw, k0[q], ray.p1, ray.p2, p3, ray.c, s);
        re[q] = fma(ray.a, at.cs, re[q]);
        im[q] = fma(ray.a, at.sn, im[q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kPsfPix; ++q) {
    const int64_t pix = (int64_t)blockIdx.x * kPsfTile + q * kPsfBlock + t;
    if (pix < npix) {
      double* o = slab + ((((size_t)b * planes + f) * slices + slice) * npix + pix) * 2;
      o[0] = re[q];
      o[1] = im[q];
    }
  }
}

// image_out: (group, plane, wavelength, pixel)
__global__ void __launch_bounds__(PRT_BLOCK)
k_psff_fold(const double* __restrict__ slab, int slices, int buckets, int64_t npix, PsfLambda lambda, int n_focus,
            int first, int planes, const double* __restrict__ norm, double* __restrict__ image_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)buckets * planes * npix) return;
  const int64_t cell = item / npix, pix = item - cell * npix;  // cell = bucket * planes + plane
  const int b = (int)(cell / planes), f = (int)(cell - (int64_t)b * planes);
  double re = 0.0, im = 0.0;
  for (int q = 0; q < slices; ++q) {
    const double* p = slab + (((size_t)cell * slices + q) * npix + pix) * 2;
    re += p[0];
    im += p[1];
  }
  const int g = b / lambda.n, k = b - g * lambda.n;
  const double inv = lambda.s[k];
  image_out[(((size_t)g * n_focus + first + f) * lambda.n + k) * npix + pix] =
      inv * inv * (re * re + im * im) / norm[g];  // (a group without rays: 0 / 0, NaN)
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t prt_frame_psf_focus_workspace_bytes(int64_t n_rows, int n_groups, int n_wavelengths, int n_focus) {
  if (n_focus < 1 || n_focus > PSFF_MAX_PLANES) return PRT_ERR_ARG;
  const int64_t psf = prt_frame_psf_workspace_bytes(n_rows, n_groups, n_wavelengths);
  if (psf < 0) return psf;
  // prt_frame_psf's, the sorted p3 and the shifts
  return psf + n_rows * (int64_t)sizeof(double) + (int64_t)n_focus * 8 + 64;
}

extern "C" int prt_frame_psf_focus(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                                   double generation, double rays_per_source, int n_groups, const double* opd,
                                   const double* pupil, const double* group_record, int weight_column,
                                   const double* wavelengths_um, int n_wavelengths, double world_unit_um, int nx,
                                   int ny, double du, double dv, const double* centre_uv, const double* axes,
                                   const double* focus, int n_focus, int track, double* image_out,
                                   double* strehl_out, double* record_out, double* axial_out, double* line_out,
                                   double* centres_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || n_groups < 1 || !group_record || !image_out || !strehl_out || !record_out ||
      !line_out || !centres_out || !workspace || !wavelengths_um || !centre_uv || !axes || !focus ||
      (n_rows && (!rows || !opd || !pupil || !axial_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  PsfLambda lambda;
  int rc = psf_lambda("psf_focus", wavelengths_um, n_wavelengths, world_unit_um, lambda);
  if (!rc) rc = psf_grid("psf_focus", nx, ny, du, dv, centre_uv);
  if (rc) return rc;
  if (n_focus < 1 || n_focus > PSFF_MAX_PLANES) return fail(PRT_ERR_ARG, "psf_focus: 1 to 256 focus shifts");
  for (int f = 0; f < n_focus; ++f)
    if (!std::isfinite(focus[f])) return fail(PRT_ERR_ARG, "psf_focus: focus finite");
  if (track != 0 && track != 1) return fail(PRT_ERR_ARG, "psf_focus: track 0 (the axis) or 1 (the chief line)");
  WfAxes ax;
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(axes[k])) return fail(PRT_ERR_ARG, "axes: finite");
  for (int k = 0; k < 3; ++k) { ax.a[k] = axes[k]; ax.e1[k] = axes[3 + k]; ax.e2[k] = axes[6 + k]; }
  const int64_t buckets = (int64_t)n_groups * n_wavelengths, npix = (int64_t)nx * ny;
  if (buckets > 65535) return fail(PRT_ERR_ARG, "psf_focus: n_groups * n_wavelengths <= 65535");
  if ((size_t)buckets * npix * 2 * sizeof(double) > kPsfSlabBytes)
    return fail(PRT_ERR_ARG, "psf_focus: n_groups * n_wavelengths * nx * ny * 16 bytes above the 256 MiB slab cap");
  int cus = 1;
  rc = psf_device(device, &cus);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_psf_focus_workspace_bytes): prt_frame_psf's, then the sorted p3 and the shifts
  int64_t* wave_rows = (int64_t*)workspace;
  int64_t* wave_offset = wave_rows + kWfMaxWaves;
  int64_t* bucket_total = wave_offset + kWfMaxWaves;
  int64_t* bucket_start = bucket_total + buckets;
  unsigned long long* skipped = (unsigned long long*)(bucket_start + buckets);
  int* status = (int*)(skipped + buckets);
  double* norm = (double*)(status + 2);
  PsfRay* stage = (PsfRay*)(((uintptr_t)(norm + n_groups) + 31) & ~(uintptr_t)31);
  PsfRay* sorted = stage + n_rows;
  int* bucket_of = (int*)(sorted + n_rows);
  double* sorted3 = (double*)(((uintptr_t)(bucket_of + n_rows) + 7) & ~(uintptr_t)7);
  double* focus_dev = sorted3 + n_rows;
  // one plane's plan is prt_frame_psf's: the slices, and with them the bits, never follow the planes
  PsfPlan plan = psf_plan(cus, n_rows, buckets, buckets, npix, kPsfTile, 16, 16, 3);
  const int slices = (int)plan.slices, all_waves = (int)plan.all_waves;
  // planes of a chunk: what the slab cap holds (at least one: the plan capped the slices for one), gridDim.z <= 65535
  const size_t plane_bytes = (size_t)buckets * slices * npix * 16;
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_focus, (int64_t)(kPsfSlabBytes / plane_bytes)),
                                                                 65535 / buckets));
  // the Strehl slab: k_psf_strehl's (bucket, slice, 3), the line's (bucket, slice, 3), the planes' (bucket, slice, plane, 2)
  const size_t cells = (size_t)buckets * slices;
  plan.strehl_bytes = cells * (3 + 3 + 2 * (size_t)n_focus) * sizeof(double);
  plan.slab_bytes = plane_bytes * chunk;
  PsfScratch scratch;
  rc = psf_scratch(st, plan, skipped, (size_t)buckets * 8 + 8, scratch);  // (the skips and the status word)
  if (rc) return rc;
  double* line_slab = scratch.strehl_slab + cells * 3;
  double* plane_slab = line_slab + cells * 3;
  HIP_TRY(hipMemcpyAsync(focus_dev, focus, (size_t)n_focus * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_psf_count, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                     rays_per_source, n_groups, plan.per_wave, wave_rows);
  hipLaunchKernelGGL(k_sort_positions, dim3(1), dim3(kSortScanBlock), 0, st, all_waves, wave_rows, wave_offset);
  hipLaunchKernelGGL(k_psff_stage, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                     rays_per_source, n_groups, plan.per_wave, wave_offset, opd, pupil, group_record, weight_column,
                     lambda, ax, stage, axial_out, bucket_of, scratch.counts, (int)buckets, skipped, status);
  sort_offsets(st, all_waves, (int)buckets, scratch.counts, bucket_total, bucket_start);
  hipLaunchKernelGGL(k_psff_scatter, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, wave_rows, wave_offset, bucket_of, stage,
                     axial_out, scratch.counts, bucket_start, (int)buckets, sorted, sorted3);
  hipLaunchKernelGGL(k_psf_strehl, dim3((unsigned)slices, (unsigned)buckets), dim3(kPsfBlock), 0, st, sorted,
                     (const PsfPar*)nullptr, n_rows, bucket_total, bucket_start, group_record, lambda, (int)WF_GROUP,
                     slices, 0, scratch.strehl_slab);
  // (strehl_out's first n_groups entries hold the Strehl ratio at P until k_psff_strehl_fold overwrites them)
  hipLaunchKernelGGL(k_psf_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     scratch.strehl_slab, slices, n_groups, lambda, bucket_total, skipped, record_out, strehl_out, norm);
  hipLaunchKernelGGL(k_psff_line, dim3((unsigned)slices, (unsigned)buckets), dim3(kPsfBlock), 0, st, sorted, sorted3,
                     bucket_total, bucket_start, slices, line_slab);
  hipLaunchKernelGGL(k_psff_line_fold, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     line_slab, slices, n_groups, n_wavelengths, track, line_out);
  const unsigned cell_blocks = (unsigned)(((int64_t)n_groups * n_focus + PRT_BLOCK - 1) / PRT_BLOCK);
  hipLaunchKernelGGL(k_psff_centres, dim3(cell_blocks), dim3(PRT_BLOCK), 0, st, line_out, focus_dev, n_groups, n_focus,
                     centre_uv[0], centre_uv[1], centres_out);
  hipLaunchKernelGGL(k_psff_strehl, dim3((unsigned)slices, (unsigned)buckets, (unsigned)n_focus), dim3(kPsfBlock), 0, st,
                     sorted, sorted3, bucket_total, bucket_start, group_record, line_out, focus_dev, lambda, slices,
                     n_focus, plane_slab);
  hipLaunchKernelGGL(k_psff_strehl_fold, dim3(cell_blocks), dim3(PRT_BLOCK), 0, st, plane_slab, slices, n_groups,
                     n_focus, lambda, norm, strehl_out);
  for (int first = 0; first < n_focus; first += chunk) {
    const int planes = std::min(chunk, n_focus - first);
    hipLaunchKernelGGL(k_psff_huygens, dim3((unsigned)plan.tiles, (unsigned)slices, (unsigned)(buckets * planes)),
                       dim3(kPsfBlock), 0, st, sorted, sorted3, bucket_total, bucket_start, group_record, focus_dev,
                       centres_out, lambda, nx, ny, du, dv, slices, n_focus, first, planes, scratch.slab);
    hipLaunchKernelGGL(k_psff_fold, dim3((unsigned)((buckets * planes * npix + PRT_BLOCK - 1) / PRT_BLOCK)),
                       dim3(PRT_BLOCK), 0, st, scratch.slab, slices, (int)buckets, npix, lambda, n_focus, first, planes,
                       norm, image_out);
  }
  int host_status;
  rc = psf_finish(st, status, scratch, &host_status);
  if (rc) return rc;
  if (host_status & PSF_BAD_WAVELENGTH)
    return fail(PRT_ERR_ARG, "psf_focus: a selected row's wavelength is not in the list");
  return PRT_OK;
}

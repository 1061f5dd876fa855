// prt_vector_psf.hpp -- the polarised diffraction PSF: the Huygens sum of prt_psf.hpp with the complex field vectors of
// prt_fresnel.hpp / prt_coatings.hpp as the rays' amplitudes.  Definitions: include/prt.h.
// It stands on prt_psf.hpp's Huygens core (the wavelength list, the plan, the scratch, psf_wavelength, psf_keep, psf_place,
// psf_slice, psf_pixel, psf_phase), reuses k_psf_count and sorts by prt_sort.hpp as the scalar pass does; the rays are
// sorted into (group, wavelength) buckets exactly as there, and the one or two states of a ray lie in planes of n_rows
// rays, so a (group, wavelength, state) bucket is the bucket's range in the state's plane.
//
//   k_vpsf_stage    per selected row, in row order: p1, p2, c = (OPD - R) s and, per state, the amplitude sqrt(w) E
//                   projected once on (e1, e2, a); beside it sqrt(w) and |E|^2; rays left out counted (integer atomics)
//   k_vpsf_scatter  the stable counting sort (psf_place) on the 72-byte rays, state by state
//   k_vpsf_strehl   per (ray slice, bucket): the six sums of c_k exp(2 pi i OPD s) in fp64, sum sqrt(w), sum |A|,
//                   sum w |E|^2 and sum w, a fixed tree order
//   k_vpsf_record   per group: the slices folded in order, the record, the two Strehl ratios, the throughput, D_g
//   k_vpsf_huygens  per (pixel tile, ray slice, bucket): three complex amplitude sums of the slice's rays at every
//                   pixel of the tile, the rays walked through LDS; partial sums into a slab of its own
//   k_vpsf_fold     per (group, wavelength, pixel): the slices added in slice order, S0..S3 and the axial part per
//                   state, the mean over the states, normalised
// No floating-point atomics: every output is the same, bit for bit, on every run.
#pragma once

enum { VPSF_RECORD = 6, VPSF_STREHL = 4, VPSF_SUMS = 10, VPSF_PLANES = 5 };
static const int kVpsfPix = 4;                      // pixels a thread owns (3 x 2 fp64 accumulators each, in registers)
static const int kVpsfTile = kPsfBlock * kVpsfPix;  // pixels of a workgroup
static const int kVpsfPixelBytes = 48;              // a pixel of the partial-sum slab: 6 doubles

struct VpsfRay { double p1, p2, c, re[3], im[3]; };  // 72 bytes; re / im: the amplitude along (e1, e2, a)
struct VpsfSide { double a, n2; };                   // sqrt(w) and |E|^2 of the ray's state
struct VpsfAxes { double e[3][3]; };                 // e1, e2, a

__global__ void __launch_bounds__(PRT_BLOCK)
k_vpsf_stage(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface, double generation,
             double rays_per_source, int n_groups, int64_t per_wave, const int64_t* __restrict__ wave_offset,
             const double* __restrict__ opd, const double* __restrict__ pupil, const double* __restrict__ group_record,
             int weight_column, PsfLambda lambda, const double* __restrict__ field, int64_t field_ld, int field_planes,
             int n_states, VpsfAxes axes, VpsfRay* __restrict__ stage, VpsfSide* __restrict__ stage_side,
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
      const int k = psf_wavelength(lambda, rows[PRT_COL_WAVELENGTH * ld + j]);
      if (k < 0) {
        atomicOr(status, PSF_BAD_WAVELENGTH);
      } else {
        const double* g = group_record + (size_t)group * WF_GROUP;
        const double o = opd[pos], x = pupil[2 * pos], y = pupil[2 * pos + 1];
        const double w = weight_column >= 0 ? rows[(int64_t)weight_column * ld + j] : 1.0;
        double er[2][3], ei[2][3];
        bool finite = true;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            er[s][q] = s < n_states ? field[(int64_t)(3 * s + q) * field_ld + j] : 0.0;
            ei[s][q] = s < n_states && field_planes == 12 ? field[(int64_t)(6 + 3 * s + q) * field_ld + j] : 0.0;
            finite = finite && fabs(er[s][q]) < PRT_INF && fabs(ei[s][q]) < PRT_INF;  // (false for a NaN)
          }
        if (psf_keep(o, x, y, w) && finite) {
          bucket = group * lambda.n + k;
          const double rho = g[5], sl = lambda.s[k], a = sqrt(w);
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            if (s >= n_states) break;
            VpsfRay ray;
            ray.p1 = x * rho;
            ray.p2 = y * rho;
            ray.c = (o - g[3]) * sl;
            double n2 = 0.0;
#pragma unroll
            for (int q = 0; q < 3; ++q) n2 += er[s][q] * er[s][q] + ei[s][q] * ei[s][q];
#pragma unroll
            for (int q = 0; q < 3; ++q) {  // (A = sqrt(w) E, then its plain dot products with the axes)
              ray.re[q] = a * er[s][0] * axes.e[q][0] + a * er[s][1] * axes.e[q][1] + a * er[s][2] * axes.e[q][2];
              ray.im[q] = a * ei[s][0] * axes.e[q][0] + a * ei[s][1] * axes.e[q][1] + a * ei[s][2] * axes.e[q][2];
            }
            stage[(int64_t)s * n_rows + pos] = ray;
            stage_side[(int64_t)s * n_rows + pos] = VpsfSide{a, n2};
          }
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
k_vpsf_scatter(const int64_t* __restrict__ wave_rows, const int64_t* __restrict__ wave_offset,
               const int* __restrict__ bucket_of, const VpsfRay* __restrict__ stage,
               const VpsfSide* __restrict__ stage_side, int64_t* __restrict__ offsets,
               const int64_t* __restrict__ bucket_start, int buckets, int64_t n_rows,
               int n_states, VpsfRay* __restrict__ sorted, VpsfSide* __restrict__ sorted_side) {
  const int64_t wave = sort_wave();
  const int64_t from = wave_offset[wave];  // (offsets + wave * buckets: only this wave reads and writes there)
  psf_place(from, from + wave_rows[wave], bucket_of, offsets + wave * buckets, bucket_start, [&](int64_t r, int64_t pos) {
    for (int s = 0; s < n_states; ++s) {
      sorted[(int64_t)s * n_rows + pos] = stage[(int64_t)s * n_rows + r];
      sorted_side[(int64_t)s * n_rows + pos] = stage_side[(int64_t)s * n_rows + r];
    }
  });
}

// bucket = (group * n_wavelengths + wavelength) * n_states + state
__global__ void __launch_bounds__(kPsfBlock)
k_vpsf_strehl(const VpsfRay* __restrict__ sorted, const VpsfSide* __restrict__ sorted_side, int64_t n_rows,
              int n_states, const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
              const double* __restrict__ group_record, PsfLambda lambda, int slices, double* __restrict__ strehl_slab) {
  __shared__ double red[VPSF_SUMS][kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.x, b = blockIdx.y;
  const int gl = b / n_states, state = b - gl * n_states, g = gl / lambda.n;
  const double s = lambda.s[gl - g * lambda.n], radius = group_record[(size_t)g * WF_GROUP + 3];
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, gl, slice, slices, lo, hi);
  const VpsfRay* const rays = sorted + (int64_t)state * n_rows;
  const VpsfSide* const sides = sorted_side + (int64_t)state * n_rows;
  double sum[VPSF_SUMS];
  for (int k = 0; k < VPSF_SUMS; ++k) sum[k] = 0.0;
  for (int64_t r = lo + t; r < hi; r += kPsfBlock) {
    const VpsfRay ray = rays[r];
    const VpsfSide side = sides[r];
    double sn, cs;
    psf_chief_phase(radius, s, ray.c, sn, cs);
    for (int k = 0; k < 3; ++k) {
      sum[2 * k] += ray.re[k] * cs - ray.im[k] * sn;
      sum[2 * k + 1] += ray.re[k] * sn + ray.im[k] * cs;
    }
    sum[6] += side.a;
    sum[7] += side.a * sqrt(side.n2);
    sum[8] += side.a * side.a * side.n2;
    sum[9] += side.a * side.a;
  }
  for (int k = 0; k < VPSF_SUMS; ++k) red[k][t] = sum[k];
  sort_tree(red, t);
  if (t < VPSF_SUMS) strehl_slab[((size_t)b * slices + slice) * VPSF_SUMS + t] = red[t][0];
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_vpsf_record(const double* __restrict__ strehl_slab, int slices, int n_groups, int n_states, PsfLambda lambda,
              const int64_t* __restrict__ bucket_total, const unsigned long long* __restrict__ skipped,
              double* __restrict__ record_out, double* __restrict__ strehl_out, double* __restrict__ norm) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  double numerator = 0.0, parallel = 0.0, aligned = 0.0, passed = 0.0, launched = 0.0;
  for (int k = 0; k < lambda.n; ++k) {
    const int gl = g * lambda.n + k;
    const double inv = lambda.s[k];
    for (int state = 0; state < n_states; ++state) {
      const int b = gl * n_states + state;
      double sum[VPSF_SUMS];
      for (int j = 0; j < VPSF_SUMS; ++j) sum[j] = 0.0;
      for (int q = 0; q < slices; ++q) {
        const double* p = strehl_slab + ((size_t)b * slices + q) * VPSF_SUMS;
        for (int j = 0; j < VPSF_SUMS; ++j) sum[j] += p[j];
      }
      double square = 0.0;
      for (int j = 0; j < 6; ++j) square += sum[j] * sum[j];
      const double num = inv * inv * square;
      double* o = record_out + (size_t)b * VPSF_RECORD;
      o[0] = (double)bucket_total[gl];
      o[1] = (double)skipped[gl];
      o[2] = sum[6];
      o[3] = sum[7];
      o[4] = num;
      o[5] = sum[8];
      numerator += num;
      aligned += (inv * sum[7]) * (inv * sum[7]);
      passed += sum[8];
      if (state == 0) {  // (the rays and their weights are the same in every state)
        parallel += (inv * sum[6]) * (inv * sum[6]);
        launched += sum[9];
      }
    }
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll), states = (double)n_states;
  numerator /= states;
  aligned /= states;
  passed /= states;
  norm[g] = parallel;
  double* o = strehl_out + (size_t)g * VPSF_STREHL;
  o[0] = parallel > 0.0 ? numerator / parallel : nan;
  o[1] = aligned > 0.0 ? numerator / aligned : nan;
  o[2] = launched > 0.0 ? passed / launched : nan;
  o[3] = parallel;
}

__global__ void __launch_bounds__(kPsfBlock)
k_vpsf_huygens(const VpsfRay* __restrict__ sorted, int64_t n_rows, int n_states,
               const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
               const double* __restrict__ group_record, PsfLambda lambda, int nx, int ny, double du, double dv,
               double u0, double v0, int slices, double* __restrict__ slab) {
  __shared__ VpsfRay tile[kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.y, b = blockIdx.z;
  const int gl = b / n_states, state = b - gl * n_states, g = gl / lambda.n;
  const double s = lambda.s[gl - g * lambda.n], radius = group_record[(size_t)g * WF_GROUP + 3];
  const int64_t npix = (int64_t)nx * ny;
  double mu[kVpsfPix], mv[kVpsfPix], k0[kVpsfPix], re[3][kVpsfPix], im[3][kVpsfPix];
#pragma unroll
  for (int q = 0; q < kVpsfPix; ++q) {
    double u, v;
    psf_pixel((int64_t)blockIdx.x * kVpsfTile + q * kPsfBlock + t, npix, nx, ny, du, dv, u0, v0, u, v);
    mu[q] = -2.0 * u;
    mv[q] = -2.0 * v;
    k0[q] = radius * radius + u * u + v * v;
#pragma unroll
    for (int k = 0; k < 3; ++k) re[k][q] = im[k][q] = 0.0;
  }
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, gl, slice, slices, lo, hi);
  const VpsfRay* const rays = sorted + (int64_t)state * n_rows;
  for (int64_t base = lo; base < hi; base += kPsfBlock) {
    __syncthreads();  // (the previous tile is read)
    if (base + t < hi) tile[t] = rays[base + t];
    __syncthreads();
    const int count = hi - base < kPsfBlock ? (int)(hi - base) : kPsfBlock;
    for (int r = 0; r < count; ++r) {
      const VpsfRay ray = tile[r];
#pragma unroll
      for (int q = 0; q < kVpsfPix; ++q) {
        const PsfPhase at = psf_phase(mu[q], mv[q], k0[q], ray.p1, ray.p2, ray.c, s);
        const double cs = at.cs, sn = at.sn;
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // (re + i im) += (ray.re + i ray.im)(cs + i sn)
          re[k][q] = fma(ray.re[k], cs, fma(-ray.im[k], sn, re[k][q]));
          im[k][q] = fma(ray.re[k], sn, fma(ray.im[k], cs, im[k][q]));
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kVpsfPix; ++q) {
    const int64_t pix = (int64_t)blockIdx.x * kVpsfTile + q * kPsfBlock + t;
    if (pix < npix) {
      double* o = slab + (((size_t)b * slices + slice) * npix + pix) * 6;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        o[2 * k] = re[k][q];
        o[2 * k + 1] = im[k][q];
      }
    }
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_vpsf_fold(const double* __restrict__ slab, int slices, int group_waves, int n_states, int64_t npix, PsfLambda lambda,
            const double* __restrict__ norm, double* __restrict__ stokes_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)group_waves * npix) return;
  const int gl = (int)(item / npix);
  const int64_t pix = item - (int64_t)gl * npix;
  double plane[VPSF_PLANES] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int state = 0; state < n_states; ++state) {
    const int b = gl * n_states + state;
    double u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < slices; ++q) {
      const double* p = slab + (((size_t)b * slices + q) * npix + pix) * 6;
      for (int k = 0; k < 6; ++k) u[k] += p[k];
    }
    const double i1 = u[0] * u[0] + u[1] * u[1], i2 = u[2] * u[2] + u[3] * u[3], i3 = u[4] * u[4] + u[5] * u[5];
    plane[0] += i1 + i2;
    plane[1] += i1 - i2;
    plane[2] += 2.0 * (u[0] * u[2] + u[1] * u[3]);  // conj(U1) U2
    plane[3] += 2.0 * (u[0] * u[3] - u[1] * u[2]);
    plane[4] += i3;
  }
  const int g = gl / lambda.n;
  const double inv = lambda.s[gl - g * lambda.n], states = (double)n_states;
  for (int k = 0; k < VPSF_PLANES; ++k)  // (a group without rays: 0 / 0, NaN)
    stokes_out[((size_t)gl * VPSF_PLANES + k) * npix + pix] = inv * inv * plane[k] / states / norm[g];
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t prt_frame_vector_psf_workspace_bytes(int64_t n_rows, int n_groups, int n_wavelengths, int n_states) {
  if (n_rows < 0 || n_groups < 1 || n_wavelengths < 1 || n_wavelengths > PSF_MAX_WAVELENGTHS ||
      (n_states != 1 && n_states != 2))
    return PRT_ERR_ARG;
  // wave counts and offsets, bucket totals / starts / skips, the status word, the groups' normalisation, per state the
  // staged and the sorted rays with what lies beside them, the rays' buckets
  return (int64_t)2 * kWfMaxWaves * 8 + 3 * psf_buckets_bytes(n_groups, n_wavelengths) + 8 + (int64_t)n_groups * 8 +
         n_rows * (int64_t)(2 * n_states * (sizeof(VpsfRay) + sizeof(VpsfSide)) + sizeof(int)) + 64;
}

extern "C" int prt_frame_vector_psf(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                                    double generation, double rays_per_source, int n_groups, const double* opd,
                                    const double* pupil, const double* group_record, int weight_column,
                                    const double* wavelengths_um, int n_wavelengths, double world_unit_um, int nx,
                                    int ny, double du, double dv, const double* centre_uv, const double* field,
                                    int64_t field_ld, int field_planes, int n_states, const double* axes,
                                    double* stokes_out, double* strehl_out, double* record_out, void* workspace,
                                    void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || n_groups < 1 || !group_record || !stokes_out || !strehl_out || !record_out ||
      !workspace || !wavelengths_um || !centre_uv || !axes || (n_rows && (!rows || !opd || !pupil || !field)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  if (field_planes != 6 && field_planes != 12)
    return fail(PRT_ERR_ARG, "vector psf: field_planes is 6 (real fields) or 12 (real parts, then imaginary parts)");
  if (n_states != 1 && n_states != 2) return fail(PRT_ERR_ARG, "vector psf: n_states is 1 (Ea) or 2 (Ea and Eb)");
  if (field_ld < n_rows) return fail(PRT_ERR_ARG, "vector psf: field_ld below n_rows");
  VpsfAxes frame;  // (the wavefront's order is a, e1, e2)
  for (int k = 0; k < 3; ++k) {
    if (!(std::isfinite(axes[k]) && std::isfinite(axes[3 + k]) && std::isfinite(axes[6 + k])))
      return fail(PRT_ERR_ARG, "vector psf: axes finite");
    frame.e[0][k] = axes[3 + k];
    frame.e[1][k] = axes[6 + k];
    frame.e[2][k] = axes[k];
  }
  PsfLambda lambda;
  int rc = psf_lambda("vector psf", wavelengths_um, n_wavelengths, world_unit_um, lambda);
  if (!rc) rc = psf_grid("psf", nx, ny, du, dv, centre_uv);
  if (rc) return rc;
  const int64_t group_waves = (int64_t)n_groups * n_wavelengths, buckets = group_waves * n_states;
  const int64_t npix = (int64_t)nx * ny;
  if (buckets > 65535) return fail(PRT_ERR_ARG, "vector psf: n_groups * n_wavelengths * n_states <= 65535");
  if ((size_t)buckets * npix * kVpsfPixelBytes > kPsfSlabBytes)
    return fail(PRT_ERR_ARG,
                "vector psf: n_groups * n_wavelengths * n_states * nx * ny * 48 bytes above the 256 MiB slab cap");
  int cus = 1;
  rc = psf_device(device, &cus);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_vector_psf_workspace_bytes)
  int64_t* wave_rows = (int64_t*)workspace;
  int64_t* wave_offset = wave_rows + kWfMaxWaves;
  int64_t* bucket_total = wave_offset + kWfMaxWaves;
  int64_t* bucket_start = bucket_total + group_waves;
  unsigned long long* skipped = (unsigned long long*)(bucket_start + group_waves);
  int* status = (int*)(skipped + group_waves);
  double* norm = (double*)(status + 2);
  VpsfRay* stage = (VpsfRay*)(((uintptr_t)(norm + n_groups) + 31) & ~(uintptr_t)31);
  VpsfRay* sorted = stage + n_states * n_rows;
  VpsfSide* stage_side = (VpsfSide*)(sorted + n_states * n_rows);
  VpsfSide* sorted_side = stage_side + n_states * n_rows;
  int* bucket_of = (int*)(sorted_side + n_states * n_rows);
  const PsfPlan plan =
      psf_plan(cus, n_rows, group_waves, buckets, npix, kVpsfTile, kVpsfPixelBytes, kVpsfPixelBytes, VPSF_SUMS);
  const int slices = (int)plan.slices, all_waves = (int)plan.all_waves;
  PsfScratch scratch;
  rc = psf_scratch(st, plan, skipped, (size_t)group_waves * 8 + 8, scratch);  // (the skips and the status word)
  if (rc) return rc;
  hipLaunchKernelGGL(k_psf_count, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                     rays_per_source, n_groups, plan.per_wave, wave_rows);
  hipLaunchKernelGGL(k_sort_positions, dim3(1), dim3(kSortScanBlock), 0, st, all_waves, wave_rows, wave_offset);
  hipLaunchKernelGGL(k_vpsf_stage, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                     rays_per_source, n_groups, plan.per_wave, wave_offset, opd, pupil, group_record, weight_column, lambda,
                     field, field_ld, field_planes, n_states, frame, stage, stage_side, bucket_of, scratch.counts,
                     (int)group_waves, skipped, status);
  sort_offsets(st, all_waves, (int)group_waves, scratch.counts, bucket_total, bucket_start);
  hipLaunchKernelGGL(k_vpsf_scatter, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, wave_rows, wave_offset, bucket_of, stage,
                     stage_side, scratch.counts, bucket_start, (int)group_waves, n_rows, n_states, sorted, sorted_side);
  hipLaunchKernelGGL(k_vpsf_strehl, dim3((unsigned)slices, (unsigned)buckets), dim3(kPsfBlock), 0, st, sorted,
                     sorted_side, n_rows, n_states, bucket_total, bucket_start, group_record, lambda, slices,
                     scratch.strehl_slab);
  hipLaunchKernelGGL(k_vpsf_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     scratch.strehl_slab, slices, n_groups, n_states, lambda, bucket_total, skipped, record_out,
                     strehl_out, norm);
  hipLaunchKernelGGL(k_vpsf_huygens, dim3((unsigned)plan.tiles, (unsigned)slices, (unsigned)buckets), dim3(kPsfBlock), 0,
                     st, sorted, n_rows, n_states, bucket_total, bucket_start, group_record, lambda, nx, ny, du, dv,
                     centre_uv[0], centre_uv[1], slices, scratch.slab);
  hipLaunchKernelGGL(k_vpsf_fold, dim3((unsigned)((group_waves * npix + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK),
                     0, st, scratch.slab, slices, (int)group_waves, n_states, npix, lambda, norm, stokes_out);
  int host_status;
  rc = psf_finish(st, status, scratch, &host_status);
  if (rc) return rc;
  if (host_status & PSF_BAD_WAVELENGTH)
    return fail(PRT_ERR_ARG, "vector psf: a selected row's wavelength is not in the list");
  return PRT_OK;
}

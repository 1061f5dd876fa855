// prt_psf_gradient.hpp -- d(PSF)/d(parameter) and d(Strehl)/d(parameter) of the diffraction PSF, on the device
// (DESIGN.md section 4.5), from the rows, the OPD, the pupil points and their derivatives that a wavefront sensitivity
// pass left there.  It stands on prt_psf.hpp: the Huygens core, the sort of prt_sort.hpp and the Strehl kernel itself -- the scalar
// PSF's is its case without parameters; the selection's checks are prt_selection.hpp's.  Definitions: include/prt.h.
//
//   k_psfg_stage      per selected row, in the selection's order: kept / missed / unfollowed, (p1, p2, c, a) and the
//                     row's (group, wavelength) bucket; per wave and bucket the rays kept; the others counted per bucket
//                     (integer atomics)
//   (k_sort_offsets, k_sort_starts of prt_sort.hpp: each wave's offset inside each bucket, each bucket's total and start)
//   k_psfg_scatter    the stable counting sort of an index: every wave writes its rays' slots, in order, at its offsets,
//                     and the staged ray beside them
//   k_psfg_stage_par  per sorted ray and parameter, gathered through the index: (e_k, q_k1, q_k2)
//   k_psf_strehl      (prt_psf.hpp) per (ray slice, bucket, quantity): sum a, sum a (cos, sin) or, for parameter k,
//                     sum a e_k (cos, sin), fp64 sincospi, a fixed tree
//   k_psfg_record     per group: the slices folded in order, the record, Strehl, dStrehl_k and the normalisation D_g
//   k_psfg_huygens<P> per (pixel tile, ray slice, bucket x chunk of P parameters): the phase path (psf_phase) once
//                     per (ray, pixel), then per parameter two multiply-adds for g_k, one product a g_k and two
//                     accumulates; the ray tile and its parameter chunk go through LDS; partial sums into a slab
//   k_psfg_fold       per (bucket, quantity, pixel): the slices added in slice order; U, dU_k, I and dI_k
// The slice count follows the selection's size, the pixel count, the bucket count and the device's CU count; a slice's
// rays follow its bucket's kept count.  Neither follows n_rows, the frame's other rows or K, and a parameter's arithmetic
// does not depend on its place in the call.  No floating-point atomics: every output is the same, bit for bit, on
// every run.
#pragma once

#include <type_traits>

enum { PSFG_MAX_PARAMETERS = 16, PSFG_RECORD = 5, PSFG_BAD_WAVELENGTH = 1, PSFG_BAD_ROW = 2 };
static const int kPsfgParams = 4;                  // parameters of a chunk at most (fp64 accumulators in registers)
static const int kPsfgQuantities = PSFG_MAX_PARAMETERS + 1;  // the slab holds U and K parameters: sized for 16
static const int kPsfgMinSlice = 2048;             // selected rows a slice should hold at least
static_assert(kPsfgMinSlice == kPsfMinSlice, "psf_plan cuts the slices of every pass by kPsfMinSlice");

__global__ void __launch_bounds__(PRT_BLOCK)
k_psfg_stage(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ selected,
             int64_t n_selected, int n_groups, const int64_t* __restrict__ group_first, const double* __restrict__ opd,
             const double* __restrict__ pupil, const double* __restrict__ groups, int weight_column, PsfLambda lambda,
             const double* __restrict__ dphase, const double* __restrict__ dpoint, int K, int64_t per_wave,
             PsfRay* __restrict__ stage, int* __restrict__ bucket_of, int64_t* __restrict__ counts, int buckets,
             unsigned long long* __restrict__ missed, unsigned long long* __restrict__ unfollowed,
             int* __restrict__ status) {
  const auto [lane, wave, first, last] = sort_run(per_wave, n_selected);
  if (first >= last) return;
  int64_t* const mine = counts + wave * buckets;  // (only this wave writes here)
  for (int64_t base = first; base < last; base += 64) {
    const int64_t r = base + lane;
    int bucket = -1;
    if (r < last) {
      const int64_t j = selected[r];
      const int group = mtf_owner(group_first, n_groups, r);
      int k = -1;
      if (j >= 0 && j < n_rows && group >= 0) {
        k = psf_wavelength(lambda, rows[PRT_COL_WAVELENGTH * ld + j]);
        if (k < 0) atomicOr(status, PSFG_BAD_WAVELENGTH);
      } else {
        atomicOr(status, PSFG_BAD_ROW);
      }
      if (k >= 0) {
        const int b = group * lambda.n + k;
        const double* g = groups + (size_t)group * 6;
        const double o = opd[r], x = pupil[2 * r], y = pupil[2 * r + 1];
        const double w = weight_column >= 0 ? rows[(int64_t)weight_column * ld + j] : 1.0;
        if (psf_keep(o, x, y, w)) {
          bool followed = true;
          for (int p = 0; p < K; ++p) {
            followed = followed && fabs(dphase[(int64_t)p * n_selected + r]) < PRT_INF;
            if (dpoint)
              followed = followed && fabs(dpoint[(int64_t)(2 * p) * n_selected + r]) < PRT_INF &&
                         fabs(dpoint[(int64_t)(2 * p + 1) * n_selected + r]) < PRT_INF;
          }
          if (followed) {
            bucket = b;
            const double rho = g[5], s = lambda.s[k];
            stage[r] = PsfRay{x * rho, y * rho, (o - g[3]) * s, sqrt(w)};
          } else {
            atomicAdd(unfollowed + b, 1ull);  // (integer: the same total in any order)
          }
        } else {
          atomicAdd(missed + b, 1ull);
        }
      }
      bucket_of[r] = bucket;
    }
    sort_tally(lane, bucket, mine);
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_psfg_scatter(int64_t n_selected, int64_t per_wave, const int* __restrict__ bucket_of,
               const PsfRay* __restrict__ stage, int64_t* __restrict__ offsets,
               const int64_t* __restrict__ bucket_start, int buckets, PsfRay* __restrict__ sorted,
               int64_t* __restrict__ order) {
  const SortRun run = sort_run(per_wave, n_selected);  // (offsets + wave * buckets: only this wave reads and writes)
  psf_place(run.first, run.last, bucket_of, offsets + run.wave * buckets, bucket_start, [&](int64_t r, int64_t pos) {
    sorted[pos] = stage[r];
    order[pos] = r;
  });
}

// per sorted ray i, slot = order[i]: e_k = dphase_k s, q_k = dpoint_k rho s (zeros without dpoint), at par[k * n_selected + i]
__global__ void __launch_bounds__(PRT_BLOCK)
k_psfg_stage_par(const double* __restrict__ rows, int64_t ld, const int64_t* __restrict__ selected, int64_t n_selected,
                 int n_groups, const int64_t* __restrict__ group_first, const double* __restrict__ groups,
                 PsfLambda lambda, const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
                 int buckets, const int64_t* __restrict__ order, const double* __restrict__ dphase,
                 const double* __restrict__ dpoint, int K, PsfPar* __restrict__ par) {
  const int64_t i = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (i >= n_selected || i >= bucket_start[buckets - 1] + bucket_total[buckets - 1]) return;
  const int64_t slot = order[i];
  const int group = mtf_owner(group_first, n_groups, slot);
  const int l = psf_wavelength(lambda, rows[PRT_COL_WAVELENGTH * ld + selected[slot]]);
  const double s = l < 0 ? 0.0 : lambda.s[l];
  const double rho = groups[(size_t)group * 6 + 5];
  for (int k = 0; k < K; ++k) {
    PsfPar p{dphase[(int64_t)k * n_selected + slot] * s, 0.0, 0.0};
    if (dpoint) {
      p.q1 = dpoint[(int64_t)(2 * k) * n_selected + slot] * rho * s;
      p.q2 = dpoint[(int64_t)(2 * k + 1) * n_selected + slot] * rho * s;
    }
    par[(int64_t)k * n_selected + i] = p;
  }
}

// Strehl = sum_l s^2 (C^2 + S^2) / D with C + i S = sum a exp(2 pi i OPD s); dStrehl_k = 2 sum_l Re(conj(U) dU_k) / D
// = 4 pi sum_l s^2 (S Ec - C Es) / D with Ec + i Es = sum a e_k exp(2 pi i OPD s)
__global__ void __launch_bounds__(PRT_BLOCK)
k_psfg_record(const double* __restrict__ strehl_slab, int slices, int n_groups, int K, PsfLambda lambda,
              const int64_t* __restrict__ bucket_total, const unsigned long long* __restrict__ missed,
              const unsigned long long* __restrict__ unfollowed, double* __restrict__ record_out,
              double* __restrict__ strehl_out, double* __restrict__ norm) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double numerator = 0.0, denominator = 0.0;
  for (int l = 0; l < lambda.n; ++l) {
    const int b = g * lambda.n + l;
    double a, c, s;
    psf_strehl_fold(strehl_slab, slices, K, b, 0, a, c, s);
    const double inv = lambda.s[l], num = inv * inv * (c * c + s * s), den = (inv * a) * (inv * a);
    double* o = record_out + (size_t)b * PSFG_RECORD;
    o[0] = (double)bucket_total[b];
    o[1] = (double)missed[b];
    o[2] = (double)unfollowed[b];
    o[3] = a;
    o[4] = den;
    numerator += num;
    denominator += den;
  }
  norm[g] = denominator;
  double* out = strehl_out + (size_t)g * (1 + K);
  out[0] = denominator > 0.0 ? numerator / denominator : nan;
  const double four_pi = 12.566370614359172;
  for (int k = 0; k < K; ++k) {
    double sum = 0.0;
    for (int l = 0; l < lambda.n; ++l) {
      const int b = g * lambda.n + l;
      double a, c, s, ec, es;
      psf_strehl_fold(strehl_slab, slices, K, b, 0, a, c, s);
      psf_strehl_fold(strehl_slab, slices, K, b, 1 + k, a, ec, es);
      const double inv = lambda.s[l];
      sum += inv * inv * (s * ec - c * es);
    }
    out[1 + k] = denominator > 0.0 ? four_pi * sum / denominator : nan;
  }
}

// Each thread owns kPsfPix pixels of the tile and, for each, the accumulators of P parameters [first, first + P) (those
// past K are zeros that are not stored).  The workgroup whose chunk starts at parameter 0 also sums U, as
// k_psf_huygens does and through the same psf_pixel and psf_phase.
// slab: (bucket, slice, quantity, pixel, 2), quantity 0 is sum a (cos, sin), 1 + k is sum a g_k (sin, cos).
template <int P>
__global__ void __launch_bounds__(kPsfBlock)
k_psfg_huygens(const PsfRay* __restrict__ sorted, const PsfPar* __restrict__ par, int64_t n_items,
              const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
              const double* __restrict__ groups, PsfLambda lambda, int K, int first_parameter, int chunks,
              int nx, int ny, double du, double dv, double u0, double v0, int slices, double* __restrict__ slab) {
  __shared__ PsfRay tile[kPsfBlock];
  __shared__ PsfPar tile_par[P][kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.y;
  const int b = (int)blockIdx.z / chunks, first = first_parameter + ((int)blockIdx.z - b * chunks) * P;
  const bool head = first == 0;
  const int g = b / lambda.n;
  const double s = lambda.s[b - g * lambda.n], radius = groups[(size_t)g * 6 + 3];
  const int64_t npix = (int64_t)nx * ny;
  double mu[kPsfPix], mv[kPsfPix], k0[kPsfPix], re[kPsfPix], im[kPsfPix], are[kPsfPix][P], aim[kPsfPix][P];
#pragma unroll
  for (int q = 0; q < kPsfPix; ++q) {
    double u, v;
    psf_pixel((int64_t)blockIdx.x * kPsfTile + q * kPsfBlock + t, npix, nx, ny, du, dv, u0, v0, u, v);
    mu[q] = -2.0 * u;
    mv[q] = -2.0 * v;
    k0[q] = radius * radius + u * u + v * v;
    re[q] = im[q] = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) are[q][j] = aim[q][j] = 0.0;
  }
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, b, slice, slices, lo, hi);
  for (int64_t base = lo; base < hi; base += kPsfBlock) {
    const int count = hi - base < kPsfBlock ? (int)(hi - base) : kPsfBlock;
    __syncthreads();  // (the previous tile is read)
    if (t < count) {
      tile[t] = sorted[base + t];
#pragma unroll
      for (int j = 0; j < P; ++j)
        tile_par[j][t] = first + j < K ? par[(int64_t)(first + j) * n_items + base + t] : PsfPar{0.0, 0.0, 0.0};
    }
    __syncthreads();
    for (int r = 0; r < count; ++r) {
      const PsfRay ray = tile[r];
#pragma unroll
      for (int q = 0; q < kPsfPix; ++q) {
        const PsfPhase at = psf_phase(mu[q], mv[q], k0[q], ray.p1, ray.p2, ray.c, s);
        if (head) {
          re[q] = fma(ray.a, at.cs, re[q]);
          im[q] = fma(ray.a, at.sn, im[q]);
        }
        const double hu = (0.5 * mu[q]) * at.inverse, hv = (0.5 * mv[q]) * at.inverse;  // -u / d, -v / d
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const PsfPar p = tile_par[j][r];
          const double ag = ray.a * fma(hu, p.q1, fma(hv, p.q2, p.e));  // a g_k, g_k = e_k - (u q_k1 + v q_k2) / d
          are[q][j] = fma(ag, at.sn, are[q][j]);
          aim[q][j] = fma(ag, at.cs, aim[q][j]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kPsfPix; ++q) {
    const int64_t pix = (int64_t)blockIdx.x * kPsfTile + q * kPsfBlock + t;
    if (pix < npix) {
      double* o = slab + ((((size_t)b * slices + slice) * (K + 1)) * npix + pix) * 2;
      if (head) {
        o[0] = re[q];
        o[1] = im[q];
      }
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (first + j < K) {
          o[(size_t)(1 + first + j) * npix * 2] = are[q][j];
          o[(size_t)(1 + first + j) * npix * 2 + 1] = aim[q][j];
        }
    }
  }
}

// U = s (sum a cos, sum a sin); dU_k = 2 pi i s sum a g_k (cos + i sin) = 2 pi s (-sum a g_k sin, sum a g_k cos);
// I = |U|^2 / D_g as k_psf_fold forms it; dI_k = 2 Re(conj(U) dU_k) / D_g
__global__ void __launch_bounds__(PRT_BLOCK)
k_psfg_fold(const double* __restrict__ slab, int slices, int buckets, int K, int64_t npix, PsfLambda lambda,
            const double* __restrict__ norm, double* __restrict__ amplitude_out, double* __restrict__ damplitude_out,
            double* __restrict__ image_out, double* __restrict__ dimage_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)buckets * (K + 1) * npix) return;
  const int b = (int)(item / ((K + 1) * npix));
  const int quantity = (int)((item - (int64_t)b * (K + 1) * npix) / npix);
  const int64_t pix = item - ((int64_t)b * (K + 1) + quantity) * npix;
  double re = 0.0, im = 0.0, are = 0.0, aim = 0.0;
  for (int q = 0; q < slices; ++q) {
    const double* p = slab + ((((size_t)b * slices + q) * (K + 1)) * npix + pix) * 2;
    re += p[0];
    im += p[1];
    if (quantity) {
      are += p[(size_t)quantity * npix * 2];
      aim += p[(size_t)quantity * npix * 2 + 1];
    }
  }
  const int g = b / lambda.n, l = b - g * lambda.n;
  const double inv = lambda.s[l], d = norm[g];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool lit = d > 0.0;  // (a group without kept rays, or without weight: NaN)
  if (quantity == 0) {
    amplitude_out[((int64_t)b * npix + pix) * 2] = lit ? inv * re : nan;
    amplitude_out[((int64_t)b * npix + pix) * 2 + 1] = lit ? inv * im : nan;
    image_out[(int64_t)b * npix + pix] = inv * inv * (re * re + im * im) / d;
  } else {
    const double two_pi = 6.283185307179586;
    const double ure = inv * re, uim = inv * im, dre = -(two_pi * inv) * are, dim = (two_pi * inv) * aim;
    const int64_t at = (((int64_t)g * K + quantity - 1) * lambda.n + l) * npix + pix;
    damplitude_out[at * 2] = lit ? dre : nan;
    damplitude_out[at * 2 + 1] = lit ? dim : nan;
    dimage_out[at] = 2.0 * (ure * dre + uim * dim) / d;
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t prt_frame_psf_gradient_workspace_bytes(int64_t n_selected, int n_groups, int n_parameters,
                                                          int n_wavelengths) {
  if (n_selected < 0 || n_groups < 1 || n_parameters < 1 || n_parameters > PSFG_MAX_PARAMETERS || n_wavelengths < 1 ||
      n_wavelengths > PSF_MAX_WAVELENGTHS || (int64_t)n_groups * n_wavelengths > 65535 / (PSFG_MAX_PARAMETERS / kPsfgParams))
    return PRT_ERR_ARG;
  // group starts and records, bucket totals / starts / missed / unfollowed, the status word, the groups' normalisation,
  // the staged and the sorted rays, the sort's index, the rays' buckets, the staged parameters
  return ((int64_t)n_groups + 1) * 8 + (int64_t)n_groups * 6 * 8 + 4 * psf_buckets_bytes(n_groups, n_wavelengths) + 8 +
         (int64_t)n_groups * 8 +
         n_selected * (int64_t)(2 * sizeof(PsfRay) + sizeof(int64_t) + sizeof(int) + (size_t)n_parameters * sizeof(PsfPar)) +
         64;
}

extern "C" int prt_frame_psf_gradient(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                                      int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                                      const double* opd, const double* pupil, const double* wavefront_groups,
                                      const double* dphase, const double* dpoint, int n_parameters,
                                      const double* wavelengths_um, int n_wavelengths, double world_unit_um, int nx,
                                      int ny, double du, double dv, const double* centre_uv, double* amplitude_out,
                                      double* damplitude_out, double* image_out, double* dimage_out, double* strehl_out,
                                      double* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  const int K = n_parameters;
  if (n_rows < 0 || ld < n_rows || n_selected < 0 || n_groups < 1 || !group_first || !wavefront_groups ||
      !amplitude_out || !damplitude_out || !image_out || !dimage_out || !strehl_out || !record_out || !workspace ||
      !wavelengths_um || !centre_uv || (n_rows && !rows))
    return fail(PRT_ERR_ARG, "psf_gradient: bad buffers");
  if (K < 1 || K > PSFG_MAX_PARAMETERS) return fail(PRT_ERR_ARG, "psf_gradient: 1 to 16 parameters");
  if (n_selected && (!selected || !opd || !pupil || !dphase))
    return fail(PRT_ERR_ARG, "psf_gradient: selected, opd, pupil and dphase where rows are selected");
  if (int bad = selection_check("psf_gradient", n_rows, n_selected, group_first, n_groups, weight_column)) return bad;
  PsfLambda lambda;
  int rc = psf_lambda("psf_gradient", wavelengths_um, n_wavelengths, world_unit_um, lambda);
  if (!rc) rc = psf_grid("psf_gradient", nx, ny, du, dv, centre_uv);
  if (rc) return rc;
  const int64_t buckets = (int64_t)n_groups * n_wavelengths, npix = (int64_t)nx * ny;
  // (the grid's z holds bucket x chunk: sized for 16 parameters whatever K is)
  if (buckets > 65535 / (PSFG_MAX_PARAMETERS / kPsfgParams))
    return fail(PRT_ERR_ARG, "psf_gradient: n_groups * n_wavelengths <= 16383");
  // the slab is sized for 16 parameters whatever K is, so that the slices do not follow K
  if ((size_t)buckets * npix * kPsfgQuantities * 16 > kPsfSlabBytes)
    return fail(PRT_ERR_ARG, "psf_gradient: n_groups * n_wavelengths * nx * ny * 17 * 16 bytes above the 256 MiB slab cap");
  int cus = 1;
  rc = psf_device(device, &cus);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_psf_gradient_workspace_bytes)
  int64_t* d_group = (int64_t*)workspace;
  double* groups = (double*)(d_group + (n_groups + 1));
  int64_t* bucket_total = (int64_t*)(groups + 6 * (size_t)n_groups);
  int64_t* bucket_start = bucket_total + buckets;
  unsigned long long* missed = (unsigned long long*)(bucket_start + buckets);
  unsigned long long* unfollowed = missed + buckets;
  int* status = (int*)(unfollowed + buckets);
  double* norm = (double*)(status + 2);
  PsfRay* stage = (PsfRay*)(((uintptr_t)(norm + n_groups) + 31) & ~(uintptr_t)31);
  PsfRay* sorted = stage + n_selected;
  int64_t* order = (int64_t*)(sorted + n_selected);
  PsfPar* par = (PsfPar*)(order + n_selected);
  int* bucket_of = (int*)(par + (size_t)K * n_selected);
  // the sort walks the selection; the slab is capped for 16 parameters and allocated for K
  const PsfPlan plan = psf_plan(cus, n_selected, buckets, buckets, npix, kPsfTile, kPsfgQuantities * 16, (K + 1) * 16,
                                (1 + K) * 3);
  const int slices = (int)plan.slices;
  if (plan.tiles > 0x7fffffff || (n_selected + PRT_BLOCK - 1) / PRT_BLOCK > 0x7fffffff ||
      (buckets * (K + 1) * npix + PRT_BLOCK - 1) / PRT_BLOCK > 0x7fffffff)
    return fail(PRT_ERR_ARG, "psf_gradient: too many rows or outputs for one launch");
  PsfScratch scratch;
  rc = psf_scratch(st, plan, missed, (size_t)buckets * 16 + 8, scratch);  // (missed, unfollowed and the status word)
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(d_group, group_first, ((size_t)n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(groups, wavefront_groups, (size_t)n_groups * 6 * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_psfg_stage, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, selected, n_selected,
                     n_groups, d_group, opd, pupil, groups, weight_column, lambda, dphase, dpoint, K, plan.per_wave, stage,
                     bucket_of, scratch.counts, (int)buckets, missed, unfollowed, status);
  sort_offsets(st, (int)plan.all_waves, (int)buckets, scratch.counts, bucket_total, bucket_start);
  hipLaunchKernelGGL(k_psfg_scatter, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, n_selected, plan.per_wave, bucket_of,
                     stage, scratch.counts, bucket_start, (int)buckets, sorted, order);
  if (n_selected)
    hipLaunchKernelGGL(k_psfg_stage_par, dim3((unsigned)((n_selected + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0,
                       st, rows, ld, selected, n_selected, n_groups, d_group, groups, lambda, bucket_total, bucket_start,
                       (int)buckets, order, dphase, dpoint, K, par);
  hipLaunchKernelGGL(k_psf_strehl, dim3((unsigned)slices, (unsigned)buckets, (unsigned)(1 + K)), dim3(kPsfBlock), 0, st,
                     sorted, par, n_selected, bucket_total, bucket_start, groups, lambda, 6, slices, K,
                     scratch.strehl_slab);
  hipLaunchKernelGGL(k_psfg_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     scratch.strehl_slab, slices, n_groups, K, lambda, bucket_total, missed, unfollowed, record_out,
                     strehl_out, norm);
  // whole chunks of kPsfgParams parameters in one launch, then the rest in the smallest instantiation that holds it
  const int whole = K / kPsfgParams, rest = K - whole * kPsfgParams;
  auto sum = [&](auto chunk, int chunks, int first) {
    hipLaunchKernelGGL(k_psfg_huygens<decltype(chunk)::value>,
                       dim3((unsigned)plan.tiles, (unsigned)slices, (unsigned)(buckets * chunks)), dim3(kPsfBlock), 0, st,
                       sorted, par, n_selected, bucket_total, bucket_start, groups, lambda, K, first, chunks, nx, ny, du,
                       dv, centre_uv[0], centre_uv[1], slices, scratch.slab);
  };
  if (whole) sum(std::integral_constant<int, kPsfgParams>(), whole, 0);
  if (rest > 2) sum(std::integral_constant<int, 4>(), 1, whole * kPsfgParams);
  else if (rest == 2) sum(std::integral_constant<int, 2>(), 1, whole * kPsfgParams);
  else if (rest == 1) sum(std::integral_constant<int, 1>(), 1, whole * kPsfgParams);
  hipLaunchKernelGGL(k_psfg_fold, dim3((unsigned)((buckets * (K + 1) * npix + PRT_BLOCK - 1) / PRT_BLOCK)),
                     dim3(PRT_BLOCK), 0, st, scratch.slab, slices, (int)buckets, K, npix, lambda, norm, amplitude_out,
                     damplitude_out, image_out, dimage_out);
  int host_status;
  rc = psf_finish(st, status, scratch, &host_status);
  if (rc) return rc;
  if (host_status & PSFG_BAD_ROW) return fail(PRT_ERR_ARG, "psf_gradient: a selected row number is outside the frame");
  if (host_status & PSFG_BAD_WAVELENGTH)
    return fail(PRT_ERR_ARG, "psf_gradient: a selected row's wavelength is not in the list");
  return PRT_OK;
}

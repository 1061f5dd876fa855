// prt_coatings.hpp -- thin-film coatings, metals and the phase of total internal reflection in the Fresnel pass
// (DESIGN.md section 4.5): complex arithmetic, the complex field vector fresnel_row (prt_fresnel.hpp) is instantiated on,
// the characteristic-matrix coefficients of a layer stack, and the tables they are read from.  Definitions: include/prt.h.
//
//   coat_stack       zs, zp of the stack at one interface, from the incidence geometry, the wavelength and the tables
//   k_coated_fresnel_step   fresnel_row on complex fields with the tables, then the counters (named apart from
//                    k_fresnel_step so that the register figure DESIGN.md states for that kernel stays that kernel's
//                    alone).  Per id: Ea, Eb as twelve planes of doubles (real parts, then imaginary parts: the first
//                    six are k_fresnel_step's layout), the previous row, the stamp: 108 bytes.
// Surfaces without a coating go through fresnel_row's one arithmetic on the real and on the imaginary parts, so a frame
// without coatings and with a real input polarisation gives k_fresnel_step's bits.
// The tables.  surface -> coating and coating -> (layers, substrate?) travel in the kernel's arguments: they are
// wave-uniform and read with scalar loads.  Thicknesses, wavelengths and the complex indices per (coating, slot,
// wavelength) lie in global memory and are read through the caches, NOT staged in LDS: at the caps they are
// 16 * 18 * 256 * 16 B = 1.2 MB, which no workgroup's 160 KB of LDS holds; what a frame really uses (a few coatings, a few
// wavelengths: some KB) stays in the vector L1 and L2; a lane's address depends on its own coating and wavelength, so
// LDS would be read with the same divergent addresses; and a workgroup of 256 rows would first copy the table it then
// reads at most 18 entries a lane of.
// The layer loop runs per lane over its own coating's layers, at most PRT_COATING_MAX_LAYERS (the count is clamped):
// lanes of other coatings, with fewer layers, or on uncoated surfaces are masked off by the compiler's exec handling;
// nothing in the loop is wave-collective.  The ballots of the counters come after all divergent code.
#pragma once

enum { COATING_MAX_SURFACES = 64, COATING_MAX_COATINGS = 16, COATING_MAX_LAYERS = 16, COATING_MAX_WAVELENGTHS = 256,
       COATING_SLOTS = COATING_MAX_LAYERS + 2 };  // ambient, the layers, substrate

struct Cx { double re, im; };
struct CxVec { FrVec re, im; };
struct CoatCoefficients { Cx zs, zp; bool tir, invalid, found; };  // (found: the row's wavelength is in the table)
struct CoatingTables {
  using Coefficients = CoatCoefficients;
  int n_coated, n_wavelengths;
  double coated[COATING_MAX_SURFACES];
  int coating_of[COATING_MAX_SURFACES];
  int n_layers[COATING_MAX_COATINGS], has_substrate[COATING_MAX_COATINGS];
  const double *thickness, *wavelengths, *indices;  // (in the workspace)
};

__device__ __forceinline__ Cx cx_add(Cx a, Cx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ Cx cx_sub(Cx a, Cx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ Cx cx_mul(Cx a, Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Cx cx_scale(Cx a, double s) { return {a.re * s, a.im * s}; }
__device__ __forceinline__ Cx cx_div(Cx a, Cx b) {
  const double m = b.re * b.re + b.im * b.im;
  return {(a.re * b.re + a.im * b.im) / m, (a.im * b.re - a.re * b.im) / m};
}
// the square root with a real part >= 0 (an imaginary part of -0 counts as +0)
__device__ __forceinline__ Cx cx_sqrt(Cx z) {
  const double m = sqrt(z.re * z.re + z.im * z.im);
  const double t = sqrt((m + fabs(z.re)) / 2.0);
  if (!(t > 0.0)) return {t, t};  // (zero, or NaN handed on)
  const double o = fabs(z.im) / (2.0 * t);
  const double sign = z.im < 0.0 ? -1.0 : 1.0;
  return z.re >= 0.0 ? Cx{t, sign * o} : Cx{o, sign * t};
}
// n cos(theta) in a medium of index n for the Snell invariant q = (ni sin(theta_i))^2, on the branch Im >= 0
__device__ __forceinline__ Cx cx_ncos(Cx n, double q) {
  Cx w = cx_sqrt(cx_sub(cx_mul(n, n), Cx{q, 0.0}));
  if (w.im < 0.0) w = {-w.re, -w.im};
  return w;
}
__device__ __forceinline__ bool cx_finite(Cx a) { return fabs(a.re) < PRT_INF && fabs(a.im) < PRT_INF; }

// one layer applied to (B, C) of one polarisation: (B, C) <- [[cos d, -i sin d / eta], [-i eta sin d, cos d]] (B, C)
// (the sign of i that goes with n + ik absorbing, fields as exp(-i omega t)); isind is -i sin d.  coat_stack hands in
// cos d and -i sin d times exp(-Im d), so (B, C) come out scaled by that: see there
__device__ __forceinline__ void coat_layer(Cx& b, Cx& c, Cx cosd, Cx isind, Cx eta) {
  const Cx nb = cx_add(cx_mul(cosd, b), cx_mul(cx_div(isind, eta), c));
  const Cx nc = cx_add(cx_mul(cx_mul(isind, eta), b), cx_mul(cosd, c));
  b = nb;
  c = nc;
}

// ---- the complex field vector: what fresnel_row asks of it, k_fresnel_step's operations on both parts -------------------
__device__ __forceinline__ void fr_fill(CxVec& e, double c) { fr_fill(e.re, c); fr_fill(e.im, c); }
__device__ __forceinline__ void fr_real(CxVec& e, const FrVec& r) { e = {r, {0.0, 0.0, 0.0}}; }
// (the imaginary parts lie six planes after the real ones)
__device__ __forceinline__ void fr_load(CxVec& e, const double* planes, int64_t n, int64_t i) {
  fr_load(e.re, planes, n, i);
  fr_load(e.im, planes + 6 * n, n, i);
}
__device__ __forceinline__ void fr_store(const CxVec& e, double* planes, int64_t n, int64_t i) {
  fr_store(e.re, planes, n, i);
  fr_store(e.im, planes + 6 * n, n, i);
}
__device__ __forceinline__ CxVec fr_scale(const CxVec& e, double c) { return {fr_scale(e.re, c), fr_scale(e.im, c)}; }
__device__ __forceinline__ CxVec fr_through(const CxVec& e, const FrVec& s, const FrVec& pi, const FrVec& pt, double cs,
                                            double cp) {
  return {fr_through(e.re, s, pi, pt, cs, cp), fr_through(e.im, s, pi, pt, cs, cp)};
}
__device__ __forceinline__ double fr_norm2(const CxVec& e) { return fr_dot(e.re, e.re) + fr_dot(e.im, e.im); }
__device__ __forceinline__ bool fr_polarised(CxVec& e, const double* v, const FrVec& ut) {
  const FrVec wr = fr_across(v, ut), wi = fr_across(v + 3, ut);
  const double ww = fr_dot(wr, wr) + fr_dot(wi, wi);
  const double m = sqrt(ww);
  e = {fr_over(wr, m), fr_over(wi, m)};
  return ww > PRT_FRESNEL_EPS_DIR;
}
// ... and with the complex coefficients of a stack
__device__ __forceinline__ CxVec coat_through(const CxVec& e, const FrVec& s, const FrVec& pi, const FrVec& pt, Cx cs,
                                              Cx cp) {
  const Cx fs = cx_mul(cs, Cx{fr_dot(e.re, s), fr_dot(e.im, s)}), fp = cx_mul(cp, Cx{fr_dot(e.re, pi), fr_dot(e.im, pi)});
  return {{fs.re * s.x + fp.re * pt.x, fs.re * s.y + fp.re * pt.y, fs.re * s.z + fp.re * pt.z},
          {fs.im * s.x + fp.im * pt.x, fs.im * s.y + fp.im * pt.y, fs.im * s.z + fp.im * pt.z}};
}
__device__ __forceinline__ CxVec coat_times(const CxVec& e, Cx c) {
  return {{c.re * e.re.x - c.im * e.im.x, c.re * e.re.y - c.im * e.im.y, c.re * e.re.z - c.im * e.im.z},
          {c.re * e.im.x + c.im * e.re.x, c.re * e.im.y + c.im * e.re.y, c.re * e.im.z + c.im * e.re.z}};
}

// the coating of a surface, -1 without one
__device__ __forceinline__ int coat_of(const CoatingTables& tb, double surface) {
  int coating = -1;
  for (int s = 0; s < tb.n_coated; ++s) coating = surface == tb.coated[s] ? tb.coating_of[s] : coating;
  return coating;
}

// r or t of the stack `coating` at wavelength lambda for light that arrives in the index ni at cos(theta) = ci,
// sin^2(theta) = xx, and leaves in nt; from the characteristic matrices of its layers.
// Every layer's matrix is carried scaled by exp(-Im delta) (Im delta >= 0 on the branch of cx_ncos): cosh and sinh of
// Im delta become (1 + e) / 2 and (1 - e) / 2 with e = exp(-2 Im delta), which lie in [0, 1] whatever the thickness or
// the absorption, and 1 - e comes from expm1, so a faintly absorbing or faintly evanescent layer does not lose its sinh
// to cancellation.  r is a quotient of (B, C) and does not see the common scale; t is multiplied by exp(-sum Im delta)
// at the end, which underflows to 0 for an opaque stack, as it should.  What is left to grow in (B, C) is a factor of
// at most max(|eta|, 1 / |eta|) a layer, so the squares in cx_div, where it divides by eta0 B + C, stay in range.
__device__ __forceinline__ CoatCoefficients coat_stack(const CoatingTables& tb, int coating, double lambda, double ni,
                                                       double nt, double ci, double xx, bool reflection) {
  CoatCoefficients r = {{-1.0, 0.0}, {1.0, 0.0}, false, false, false};
  if (!(lambda > 0.0 && lambda < PRT_INF)) {
    r.invalid = true;
    return r;
  }
  // (the sorted wavelengths: a lower bound in at most 8 steps, then an exact comparison)
  int lo = 0, hi = tb.n_wavelengths;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tb.wavelengths[mid] < lambda) lo = mid + 1; else hi = mid;
  }
  if (!(lo < tb.n_wavelengths && tb.wavelengths[lo] == lambda)) return r;
  r.found = true;
  const int w = lo;
  const int c = coating < COATING_MAX_COATINGS ? coating : COATING_MAX_COATINGS - 1;
  const int layers = tb.n_layers[c] < COATING_MAX_LAYERS ? tb.n_layers[c] : COATING_MAX_LAYERS;
  const double* __restrict__ table = tb.indices + ((int64_t)c * COATING_SLOTS * tb.n_wavelengths + w) * 2;
  const int64_t slot = (int64_t)tb.n_wavelengths * 2;  // (doubles from one slot to the next)
  const Cx ambient = {table[0], table[1]};
  const bool from_ambient = ni == ambient.re;
  Cx far = {nt, 0.0};
  if (reflection && from_ambient) {
    far = {table[(COATING_SLOTS - 1) * slot], table[(COATING_SLOTS - 1) * slot + 1]};
    if (!tb.has_substrate[c]) r.invalid = true;
  } else if (reflection) {
    far = ambient;
  }
  const double q = (ni * ni) * xx;  // (|ui x N|^2 = sin^2 of the angle of incidence)
  const double eta0s = ni * ci, eta0p = ni / ci;
  const Cx far_ncos = cx_ncos(far, q);
  const Cx far_s = far_ncos, far_p = cx_div(cx_mul(far, far), far_ncos);
  Cx bs = {1.0, 0.0}, cs = far_s, bp = {1.0, 0.0}, cp = far_p;
  bool finite = cx_finite(far);
  double damping = 0.0;  // (sum of Im delta over the layers)
  // (from the layer next to the far medium to the one next to the near medium)
  for (int step = 0; step < COATING_MAX_LAYERS; ++step) {
    if (step >= layers) break;
    const int l = from_ambient ? layers - 1 - step : step;
    const Cx nl = {table[(1 + l) * slot], table[(1 + l) * slot + 1]};
    const double thick = tb.thickness[c * COATING_MAX_LAYERS + l];
    finite = finite && cx_finite(nl);
    const Cx ncos = cx_ncos(nl, q);
    const Cx delta = cx_scale(ncos, 6.283185307179586 * thick / lambda);
    double sn, cn;
    sincos(delta.re, &sn, &cn);
    const double less = expm1(-2.0 * delta.im);  // (e - 1)
    const double ch = (2.0 + less) / 2.0, sh = -less / 2.0;
    damping += delta.im;
    const Cx cosd = {cn * ch, -(sn * sh)};
    const Cx isind = {cn * sh, -(sn * ch)};  // -i sin(delta), sin(a + ib) = sin a cosh b + i cos a sinh b
    coat_layer(bs, cs, cosd, isind, ncos);
    coat_layer(bp, cp, cosd, isind, cx_div(cx_mul(nl, nl), ncos));
  }
  const Cx den_s = cx_add(cx_scale(bs, eta0s), cs), den_p = cx_add(cx_scale(bp, eta0p), cp);
  if (reflection) {  // (rs; rp with the sign the basis s, pi, pt gives it: -1, +1 for a perfect conductor)
    r.zs = cx_div(cx_sub(cx_scale(bs, eta0s), cs), den_s);
    r.zp = cx_div(cx_sub(cp, cx_scale(bp, eta0p)), den_p);
    r.tir = far.im == 0.0 && far.re * far.re < q;
  } else {  // (power-normalised: sqrt(Re eta_far / eta_near))
    const double dim = exp(-damping);
    r.zs = cx_scale(cx_div(Cx{2.0 * eta0s, 0.0}, den_s), sqrt(far_s.re / eta0s) * dim);
    r.zp = cx_scale(cx_div(Cx{2.0 * eta0p, 0.0}, den_p), sqrt(far_p.re / eta0p) * dim);
  }
  if (!(finite && cx_finite(r.zs) && cx_finite(r.zp))) r.invalid = true;
  r.tir = r.tir && !r.invalid;
  return r;
}

__global__ void __launch_bounds__(kFresnelBlock)
k_coated_fresnel_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count,
                      int generation, double id0, int64_t n_ids, FresnelArgs args, CoatingTables tables,
                      double* __restrict__ field, int64_t* __restrict__ last_row, int* __restrict__ stamp,
                      FresnelWords* __restrict__ words, double* __restrict__ t_out, double* __restrict__ field_out) {
  const int64_t j = start + (int64_t)blockIdx.x * kFresnelBlock + threadIdx.x;
  bool flag[COATED_COUNTERS] = {};
  if (j < start + count)
    fresnel_row<CxVec>(rows, ld, n_rows, j, generation, id0, n_ids, args, tables, field, last_row, stamp, &words->status,
                       t_out, field_out, flag);
  fresnel_count(flag, words->count);
}

// ---- entry points ---------------------------------------------------------------------------------------------------
static const int64_t kCoatedTableBytes =
    (int64_t)sizeof(double) * (COATING_MAX_COATINGS * COATING_MAX_LAYERS + COATING_MAX_WAVELENGTHS +
                               2 * COATING_MAX_COATINGS * COATING_SLOTS * COATING_MAX_WAVELENGTHS);

extern "C" int64_t prt_frame_fresnel_coated_workspace_bytes(int64_t n_rows, int64_t n_ids) {
  return fresnel_workspace_bytes(n_rows, n_ids, kCoatedTableBytes, 12);  // (the tables at their caps)
}

// the caller's tables checked and, but for the device pointers, put into the kernel's argument
static int coat_check(const int64_t* lossless, int n_lossless, const int64_t* coated_surfaces, const int32_t* surface_coating,
                      int n_coated, int n_coatings, const int32_t* layer_counts, const int32_t* has_substrate,
                      const double* thicknesses, const double* wavelengths, int n_wavelengths, const double* indices,
                      CoatingTables& tables) {
  if (n_coated < 0 || n_coated > COATING_MAX_SURFACES || (n_coated && (!coated_surfaces || !surface_coating)))
    return fail(PRT_ERR_ARG, "coatings: at most 64 coated surfaces");
  if (n_coatings < 0 || n_coatings > COATING_MAX_COATINGS ||
      (n_coatings && (!layer_counts || !has_substrate || !thicknesses || !indices)))
    return fail(PRT_ERR_ARG, "coatings: at most 16 coatings");
  if (n_wavelengths < 0 || n_wavelengths > COATING_MAX_WAVELENGTHS || (n_wavelengths && !wavelengths))
    return fail(PRT_ERR_ARG, "coatings: at most 256 wavelengths");
  for (int w = 0; w < n_wavelengths; ++w)
    if (!(wavelengths[w] > 0.0 && wavelengths[w] < PRT_INF) || (w && !(wavelengths[w - 1] < wavelengths[w])))
      return fail(PRT_ERR_ARG, "coatings: wavelengths finite, > 0, ascending and distinct");
  std::memset(&tables, 0, sizeof(tables));
  for (int c = 0; c < n_coatings; ++c) {
    if (layer_counts[c] < 0 || layer_counts[c] > COATING_MAX_LAYERS)
      return fail(PRT_ERR_ARG, "coatings: at most 16 layers");
    for (int l = 0; l < layer_counts[c]; ++l) {
      const double thick = thicknesses[c * COATING_MAX_LAYERS + l];
      if (!(thick >= 0.0 && thick < PRT_INF)) return fail(PRT_ERR_ARG, "coatings: thicknesses finite and >= 0");
    }
    tables.n_layers[c] = layer_counts[c];
    tables.has_substrate[c] = has_substrate[c] != 0;
  }
  for (int s = 0; s < n_coated; ++s) {
    if (surface_coating[s] < 0 || surface_coating[s] >= n_coatings)
      return fail(PRT_ERR_ARG, "coatings: a surface names a coating that is not there");
    for (int r = 0; r < s; ++r)
      if (coated_surfaces[r] == coated_surfaces[s]) return fail(PRT_ERR_ARG, "coatings: a surface is listed twice");
    for (int r = 0; r < n_lossless; ++r)
      if (lossless[r] == coated_surfaces[s]) return fail(PRT_ERR_ARG, "coatings: a surface is both lossless and coated");
    tables.coated[s] = (double)coated_surfaces[s];
    tables.coating_of[s] = surface_coating[s];
  }
  tables.n_coated = n_coated;
  tables.n_wavelengths = n_wavelengths;
  return PRT_OK;
}

extern "C" int prt_frame_fresnel_coated(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                        int n_generations, double id0, int64_t n_ids, const double* polarization,
                                        const int64_t* lossless, int n_lossless, const int64_t* coated_surfaces,
                                        const int32_t* surface_coating, int n_coated, int n_coatings,
                                        const int32_t* layer_counts, const int32_t* has_substrate,
                                        const double* thicknesses, const double* wavelengths, int n_wavelengths,
                                        const double* indices, double* transmittance_out, double* field_out,
                                        int64_t* record_out, void* workspace, void* stream) {
  const FresnelCall call = {rows, ld, rows_per_generation, n_generations, id0, n_ids, polarization, lossless, n_lossless,
                            transmittance_out, record_out, workspace, stream};
  FresnelArgs args;
  CoatingTables tables;
  const int64_t n_rows = fresnel_check(call, 2, COATED_COUNTERS, args, [&] {
    return coat_check(lossless, n_lossless, coated_surfaces, surface_coating, n_coated, n_coatings, layer_counts,
                      has_substrate, thicknesses, wavelengths, n_wavelengths, indices, tables);
  });
  if (n_rows <= 0) return (int)n_rows;
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const FresnelWork w = fresnel_carve(workspace, n_ids, kCoatedTableBytes, 12);
  double* d_thickness = (double*)w.tables;
  double* d_wavelengths = d_thickness + COATING_MAX_COATINGS * COATING_MAX_LAYERS;
  double* d_indices = d_wavelengths + COATING_MAX_WAVELENGTHS;
  if (n_coatings) {
    HIP_TRY(hipMemcpyAsync(d_thickness, thicknesses, sizeof(double) * n_coatings * COATING_MAX_LAYERS,
                           hipMemcpyHostToDevice, st));
    if (n_wavelengths) {
      HIP_TRY(hipMemcpyAsync(d_wavelengths, wavelengths, sizeof(double) * n_wavelengths, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_indices, indices, sizeof(double) * 2 * n_coatings * COATING_SLOTS * n_wavelengths,
                             hipMemcpyHostToDevice, st));
    }
  }
  tables.thickness = d_thickness;
  tables.wavelengths = d_wavelengths;
  tables.indices = d_indices;
  return fresnel_run(call, n_rows, w, COATED_COUNTERS, [&](dim3 grid, int64_t start, int64_t count, int g) {
    hipLaunchKernelGGL(k_coated_fresnel_step, grid, dim3(kFresnelBlock), 0, st, rows, ld, n_rows, start, count, g, id0,
                       n_ids, args, tables, w.field, w.last_row, w.stamp, w.words, transmittance_out, field_out);
  });
}

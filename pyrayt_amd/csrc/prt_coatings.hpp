// prt_coatings.hpp -- thin-film coatings, metals and the phase of total internal reflection in the Fresnel pass
// (DESIGN.md section 4.5): k_fresnel_step's join by ray id with complex fields and, at the surfaces the caller coats,
// the characteristic-matrix coefficients of a layer stack.  Definitions: include/prt.h.
//
//   k_coated_fresnel_step   the coated step (the issue's k_fresnel_coated_step; named so that the register figure
//                    DESIGN.md states for k_fresnel_step stays that kernel's alone).  k_fresnel_step's shape: one launch
//                    per generation in order on one stream, one row a thread, the stamp exchange, the previous row's
//                    NUMBER kept per id.  Per id: Ea, Eb as twelve planes of doubles (real parts, then imaginary
//                    parts), the previous row, the stamp: 108 bytes.
// Surfaces without a coating follow k_fresnel_step's arithmetic operation for operation on the real and on the
// imaginary parts, so a frame without coatings and with a real input polarisation gives k_fresnel_step's bits.
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

enum { FRESNEL_NO_WAVELENGTH = 8 };
enum { COATING_MAX_SURFACES = 64, COATING_MAX_COATINGS = 16, COATING_MAX_LAYERS = 16, COATING_MAX_WAVELENGTHS = 256,
       COATING_SLOTS = COATING_MAX_LAYERS + 2,  // ambient, the layers, substrate
       COATED_COUNTERS = 6 };  // k_fresnel_step's four, then coated interfaces and interfaces of total internal reflection

struct CoatedWords { u64 count[COATED_COUNTERS]; int status; };  // (cleared together, read back together: 52 <= 64 bytes)
struct CoatedArgs {
  double vr[3], vi[3];
  int polarised, n_lossless, n_coated, n_wavelengths;
  double lossless[FRESNEL_MAX_LOSSLESS];
  double coated[COATING_MAX_SURFACES];
  int coating_of[COATING_MAX_SURFACES];
  int n_layers[COATING_MAX_COATINGS], has_substrate[COATING_MAX_COATINGS];
};
struct Cx { double re, im; };
struct CxVec { FrVec re, im; };

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
// (the sign of i that goes with n + ik absorbing, fields as exp(-i omega t)); isind is -i sin d
__device__ __forceinline__ void coat_layer(Cx& b, Cx& c, Cx cosd, Cx isind, Cx eta) {
  const Cx nb = cx_add(cx_mul(cosd, b), cx_mul(cx_div(isind, eta), c));
  const Cx nc = cx_add(cx_mul(cx_mul(isind, eta), b), cx_mul(cosd, c));
  b = nb;
  c = nc;
}

// E' = (cs (E.s)) s + (cp (E.pi)) pt with real coefficients: k_fresnel_step's fr_through on both parts
__device__ __forceinline__ CxVec coat_through_real(const CxVec& e, const FrVec& s, const FrVec& pi, const FrVec& pt,
                                                   double cs, double cp) {
  return {fr_through(e.re, s, pi, pt, cs, cp), fr_through(e.im, s, pi, pt, cs, cp)};
}
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
__device__ __forceinline__ double coat_norm2(const CxVec& e) { return fr_dot(e.re, e.re) + fr_dot(e.im, e.im); }

__global__ void __launch_bounds__(kFresnelBlock)
k_coated_fresnel_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count,
                      int generation, double id0, int64_t n_ids, CoatedArgs args, const double* __restrict__ thickness,
                      const double* __restrict__ wavelengths, const double* __restrict__ indices,
                      double* __restrict__ field, int64_t* __restrict__ last_row, int* __restrict__ stamp,
                      CoatedWords* __restrict__ words, double* __restrict__ t_out, double* __restrict__ field_out) {
  __shared__ unsigned red[COATED_COUNTERS][kFresnelWaves];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t j = start + (int64_t)blockIdx.x * kFresnelBlock + threadIdx.x;
  bool reflection = false, lossless = false, undeviated = false, invalid = false, coated = false, tir = false;
  if (j < start + count) {
    const FrVec nan3 = {nan, nan, nan}, zero3 = {0.0, 0.0, 0.0};
    CxVec ea = {nan3, nan3}, eb = ea;
    double t = nan;
    const double k = rows[PRT_COL_ID * ld + j] - id0;
    int64_t i = -1;
    bool joined = false, dead = true;
    if (!(k >= 0.0 && k < (double)n_ids && k == floor(k))) {
      atomicOr(&words->status, FRESNEL_BAD_ID);
    } else {
      i = (int64_t)k;
      // (stamp: the generation that wrote the ray's state last, + 1)
      const int before = atomicExch(stamp + i, generation + 1);
      joined = before == generation;
      if (before == generation + 1) atomicOr(&words->status, FRESNEL_REPEATED_ID);
      else if (!joined) atomicOr(&words->status, FRESNEL_NOT_WHOLE);  // (no row in generation - 1)
    }
    if (joined) {
      const FrVec raw = fr_tilt(rows, ld, j);
      const double mm = fr_dot(raw, raw);
      const FrVec ut = fr_over(raw, sqrt(mm));
      if (generation == 0) {
        invalid = !(mm > 0.0 && mm < PRT_INF);
        if (!invalid && args.polarised) {
          const FrVec vr = {args.vr[0], args.vr[1], args.vr[2]}, vi = {args.vi[0], args.vi[1], args.vi[2]};
          const double along_r = fr_dot(vr, ut), along_i = fr_dot(vi, ut);
          const FrVec wr = {vr.x - along_r * ut.x, vr.y - along_r * ut.y, vr.z - along_r * ut.z};
          const FrVec wi = {vi.x - along_i * ut.x, vi.y - along_i * ut.y, vi.z - along_i * ut.z};
          const double ww = fr_dot(wr, wr) + fr_dot(wi, wi);
          invalid = !(ww > PRT_FRESNEL_EPS_DIR);
          const double m = sqrt(ww);
          ea = {fr_over(wr, m), fr_over(wi, m)};
          eb = {zero3, zero3};
        } else if (!invalid) {
          const double ax = fabs(ut.x), ay = fabs(ut.y), az = fabs(ut.z);
          int axis = 0;
          double least = ax;
          if (ay < least) { axis = 1; least = ay; }
          if (az < least) axis = 2;
          const FrVec e = {axis == 0 ? 1.0 : 0.0, axis == 1 ? 1.0 : 0.0, axis == 2 ? 1.0 : 0.0};
          ea = {fr_unit(fr_cross(ut, e)), zero3};
          eb = {fr_cross(ut, ea.re), zero3};
        }
        t = 1.0;
        dead = invalid;
      } else {
        int64_t p = last_row[i];  // (written by the launch of generation - 1: the stamp said so)
        p = p >= 0 && p < n_rows ? p : j;
        const double t_before = t_out[p];
        const FrVec ui = fr_unit(fr_tilt(rows, ld, p));
        const double ni = rows[PRT_COL_INDEX * ld + p], nt = rows[PRT_COL_INDEX * ld + j];
        const double surface = rows[PRT_COL_SURFACE * ld + p];
        for (int s = 0; s < args.n_lossless; ++s) lossless = lossless || surface == args.lossless[s];
        int coating = -1;
        for (int s = 0; s < args.n_coated; ++s) coating = surface == args.coated[s] ? args.coating_of[s] : coating;
        const FrVec d = {ui.x - ut.x, ui.y - ut.y, ui.z - ut.z};
        const double dd = fr_dot(d, d);
        t = t_before;
        bool from_fields = false, through_real = true, touched = false, normal = false;
        double cs = -1.0, cp = 1.0;
        Cx zs = {-1.0, 0.0}, zp = {1.0, 0.0};
        FrVec s = zero3, pi = zero3, pt = zero3;
        if (!(dd < PRT_INF && ni > 0.0 && ni < PRT_INF && nt > 0.0 && nt < PRT_INF)) {
          invalid = true;
        } else if (ni == nt && dd <= PRT_FRESNEL_EPS_DIR) {
          undeviated = true;
        } else {
          FrVec n;
          double ci;
          touched = true;
          reflection = ni == nt;
          if (reflection) {
            n = fr_over(d, sqrt(dd));
            ci = fr_dot(ui, n);
          } else {
            n = fr_unit({ni * ui.x - nt * ut.x, ni * ui.y - nt * ut.y, ni * ui.z - nt * ut.z});
            ci = fr_dot(ui, n);
            if (ci < 0.0) { n = {-n.x, -n.y, -n.z}; ci = -ci; }
            const double ct = fr_dot(ut, n);
            invalid = !(ci > 0.0 && ct > 0.0);
            const double a = ni * ci, b = nt * ct, c = nt * ci, e = ni * ct;
            const double twice = 2.0 * sqrt(a * b);
            cs = lossless ? 1.0 : twice / (a + b);
            cp = lossless ? 1.0 : twice / (c + e);
            from_fields = !lossless;
          }
          const FrVec x = fr_cross(ui, n);
          const double xx = fr_dot(x, x);
          normal = xx <= PRT_FRESNEL_EPS_DIR;  // (normal incidence: s and p coincide)
          if (!normal) {
            s = fr_over(x, sqrt(xx));
            pi = fr_cross(ui, s);
            pt = fr_cross(ut, s);
          }
          if (coating >= 0) {
            // ---- the coated interface: r, t of the stack from the characteristic matrices of its layers ----
            coated = true;
            through_real = false;
            from_fields = true;
            const double lambda = rows[PRT_COL_WAVELENGTH * ld + p];
            int w = -1;
            if (!(lambda > 0.0 && lambda < PRT_INF)) {
              invalid = true;
            } else {  // (the sorted wavelengths: a lower bound in at most 8 steps, then an exact comparison)
              int lo = 0, hi = args.n_wavelengths;
              while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (wavelengths[mid] < lambda) lo = mid + 1; else hi = mid;
              }
              if (lo < args.n_wavelengths && wavelengths[lo] == lambda) w = lo;
              else atomicOr(&words->status, FRESNEL_NO_WAVELENGTH);
            }
            if (w >= 0) {
              const int c = coating < COATING_MAX_COATINGS ? coating : COATING_MAX_COATINGS - 1;
              const int layers = args.n_layers[c] < COATING_MAX_LAYERS ? args.n_layers[c] : COATING_MAX_LAYERS;
              const double* __restrict__ table = indices + ((int64_t)c * COATING_SLOTS * args.n_wavelengths + w) * 2;
              const int64_t slot = (int64_t)args.n_wavelengths * 2;  // (doubles from one slot to the next)
              const Cx ambient = {table[0], table[1]};
              const bool from_ambient = ni == ambient.re;
              Cx far = {nt, 0.0};
              if (reflection && from_ambient) {
                far = {table[(COATING_SLOTS - 1) * slot], table[(COATING_SLOTS - 1) * slot + 1]};
                if (!args.has_substrate[c]) invalid = true;
              } else if (reflection) {
                far = ambient;
              }
              const double q = (ni * ni) * xx;  // (|ui x N|^2 = sin^2 of the angle of incidence)
              const double eta0s = ni * ci, eta0p = ni / ci;
              const Cx far_ncos = cx_ncos(far, q);
              const Cx far_s = far_ncos, far_p = cx_div(cx_mul(far, far), far_ncos);
              Cx bs = {1.0, 0.0}, cs_ = far_s, bp = {1.0, 0.0}, cp_ = far_p;
              bool finite = cx_finite(far);
              // (from the layer next to the far medium to the one next to the near medium)
              for (int step = 0; step < COATING_MAX_LAYERS; ++step) {
                if (step >= layers) break;
                const int l = from_ambient ? layers - 1 - step : step;
                const Cx nl = {table[(1 + l) * slot], table[(1 + l) * slot + 1]};
                const double thick = thickness[c * COATING_MAX_LAYERS + l];
                finite = finite && cx_finite(nl);
                const Cx ncos = cx_ncos(nl, q);
                const Cx delta = cx_scale(ncos, 6.283185307179586 * thick / lambda);
                double sn, cn;
                sincos(delta.re, &sn, &cn);
                const double ep = exp(delta.im), em = 1.0 / ep;
                const double ch = (ep + em) / 2.0, sh = (ep - em) / 2.0;
                const Cx cosd = {cn * ch, -(sn * sh)};
                const Cx isind = {cn * sh, -(sn * ch)};  // -i sin(delta), sin(a + ib) = sin a cosh b + i cos a sinh b
                coat_layer(bs, cs_, cosd, isind, ncos);
                coat_layer(bp, cp_, cosd, isind, cx_div(cx_mul(nl, nl), ncos));
              }
              const Cx den_s = cx_add(cx_scale(bs, eta0s), cs_), den_p = cx_add(cx_scale(bp, eta0p), cp_);
              if (reflection) {  // (rs; rp with the sign the basis s, pi, pt gives it: -1, +1 for a perfect conductor)
                zs = cx_div(cx_sub(cx_scale(bs, eta0s), cs_), den_s);
                zp = cx_div(cx_sub(cp_, cx_scale(bp, eta0p)), den_p);
                tir = far.im == 0.0 && far.re * far.re < q;
              } else {  // (power-normalised: sqrt(Re eta_far / eta_near))
                zs = cx_scale(cx_div(Cx{2.0 * eta0s, 0.0}, den_s), sqrt(far_s.re / eta0s));
                zp = cx_scale(cx_div(Cx{2.0 * eta0p, 0.0}, den_p), sqrt(far_p.re / eta0p));
              }
              if (!(finite && cx_finite(zs) && cx_finite(zp))) invalid = true;
            } else {
              through_real = true;  // (no coefficients: the row is invalid or the call refused)
              if (!invalid) touched = false;
            }
            tir = tir && !invalid;
          }
        }
        ea = {{field[i], field[n_ids + i], field[2 * n_ids + i]},
              {field[6 * n_ids + i], field[7 * n_ids + i], field[8 * n_ids + i]}};
        eb = {{field[3 * n_ids + i], field[4 * n_ids + i], field[5 * n_ids + i]},
              {field[9 * n_ids + i], field[10 * n_ids + i], field[11 * n_ids + i]}};
        if (touched && through_real) {
          if (normal) {
            ea = {{cs * ea.re.x, cs * ea.re.y, cs * ea.re.z}, {cs * ea.im.x, cs * ea.im.y, cs * ea.im.z}};
            eb = {{cs * eb.re.x, cs * eb.re.y, cs * eb.re.z}, {cs * eb.im.x, cs * eb.im.y, cs * eb.im.z}};
          } else {
            ea = coat_through_real(ea, s, pi, pt, cs, cp);
            eb = coat_through_real(eb, s, pi, pt, cs, cp);
          }
        } else if (touched) {
          if (normal) {
            ea = coat_times(ea, zs);
            eb = coat_times(eb, zs);
          } else {
            ea = coat_through(ea, s, pi, pt, zs, zp);
            eb = coat_through(eb, s, pi, pt, zs, zp);
          }
        }
        // (coefficients of magnitude 1 by definition hand the transmittance on as it is; a coated interface never does)
        if (touched && from_fields) {
          const double aa = coat_norm2(ea);
          t = args.polarised ? aa : (aa + coat_norm2(eb)) / 2.0;
        }
        dead = invalid || t_before != t_before;
        invalid = invalid && t_before == t_before;  // (a ray is counted once: it is NaN from there on)
      }
    }
    if (dead) {
      ea = {nan3, nan3};
      eb = ea;
      t = nan;
    }
    if (i >= 0) {  // (also for a row the status word refuses: what the next generation reads is this launch's own)
      field[i] = ea.re.x; field[n_ids + i] = ea.re.y; field[2 * n_ids + i] = ea.re.z;
      field[3 * n_ids + i] = eb.re.x; field[4 * n_ids + i] = eb.re.y; field[5 * n_ids + i] = eb.re.z;
      field[6 * n_ids + i] = ea.im.x; field[7 * n_ids + i] = ea.im.y; field[8 * n_ids + i] = ea.im.z;
      field[9 * n_ids + i] = eb.im.x; field[10 * n_ids + i] = eb.im.y; field[11 * n_ids + i] = eb.im.z;
      last_row[i] = j;
    }
    t_out[j] = t;
    if (field_out) {
      field_out[j] = ea.re.x; field_out[n_rows + j] = ea.re.y; field_out[2 * n_rows + j] = ea.re.z;
      field_out[3 * n_rows + j] = eb.re.x; field_out[4 * n_rows + j] = eb.re.y; field_out[5 * n_rows + j] = eb.re.z;
      field_out[6 * n_rows + j] = ea.im.x; field_out[7 * n_rows + j] = ea.im.y; field_out[8 * n_rows + j] = ea.im.z;
      field_out[9 * n_rows + j] = eb.im.x; field_out[10 * n_rows + j] = eb.im.y; field_out[11 * n_rows + j] = eb.im.z;
    }
  }
  // the counters: over the wave, over the workgroup, one atomic each
  const unsigned tally[COATED_COUNTERS] = {(unsigned)__popcll(__ballot(reflection)), (unsigned)__popcll(__ballot(lossless)),
                                           (unsigned)__popcll(__ballot(undeviated)), (unsigned)__popcll(__ballot(invalid)),
                                           (unsigned)__popcll(__ballot(coated)), (unsigned)__popcll(__ballot(tir))};
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < COATED_COUNTERS; ++c) red[c][threadIdx.x >> 6] = tally[c];
  __syncthreads();
  if (threadIdx.x < COATED_COUNTERS) {
    unsigned sum = 0;
    for (int w = 0; w < kFresnelWaves; ++w) sum += red[threadIdx.x][w];
    if (sum) atomicAdd(&words->count[threadIdx.x], (u64)sum);
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------
static const int64_t kCoatedTableBytes =
    (int64_t)sizeof(double) * (COATING_MAX_COATINGS * COATING_MAX_LAYERS + COATING_MAX_WAVELENGTHS +
                               2 * COATING_MAX_COATINGS * COATING_SLOTS * COATING_MAX_WAVELENGTHS);

extern "C" int64_t prt_frame_fresnel_coated_workspace_bytes(int64_t n_rows, int64_t n_ids) {
  if (!fresnel_sizes_ok(n_rows, n_ids)) return PRT_ERR_ARG;
  // the words; the tables at their caps; per id: Ea and Eb (twelve planes of doubles), its previous row, the stamp
  return 64 + kCoatedTableBytes + n_ids * (int64_t)(12 * sizeof(double) + sizeof(int64_t) + sizeof(int)) + 64;
}

extern "C" int prt_frame_fresnel_coated(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                        int n_generations, double id0, int64_t n_ids, const double* polarization,
                                        const int64_t* lossless, int n_lossless, const int64_t* coated_surfaces,
                                        const int32_t* surface_coating, int n_coated, int n_coatings,
                                        const int32_t* layer_counts, const int32_t* has_substrate,
                                        const double* thicknesses, const double* wavelengths, int n_wavelengths,
                                        const double* indices, double* transmittance_out, double* field_out,
                                        int64_t* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  if (n_generations < 0 || (n_generations && !rows_per_generation) || ld < 0) return fail(PRT_ERR_ARG, "bad buffers");
  int64_t n_rows = 0;
  for (int g = 0; g < n_generations; ++g) {
    if (rows_per_generation[g] < 0) return fail(PRT_ERR_ARG, "rows_per_generation: counts >= 0");
    if ((rows_per_generation[g] + kFresnelBlock - 1) / kFresnelBlock > 0x7fffffff)
      return fail(PRT_ERR_ARG, "fresnel: too many rows in a generation for one launch");
    n_rows += rows_per_generation[g];
  }
  if (ld < n_rows || !record_out || !workspace || (n_rows && (!rows || !transmittance_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(n_ids >= 1 && n_ids <= ((int64_t)1 << 31)) || !(id0 == id0 && std::fabs(id0) < 9.0e15))
    return fail(PRT_ERR_ARG, "ids: n_ids in [1, 2^31], id0 finite");
  if (n_lossless < 0 || n_lossless > FRESNEL_MAX_LOSSLESS || (n_lossless && !lossless))
    return fail(PRT_ERR_ARG, "fresnel: at most 64 lossless surfaces");
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
  CoatedArgs args;
  std::memset(&args, 0, sizeof(args));
  for (int c = 0; c < n_coatings; ++c) {
    if (layer_counts[c] < 0 || layer_counts[c] > COATING_MAX_LAYERS)
      return fail(PRT_ERR_ARG, "coatings: at most 16 layers");
    for (int l = 0; l < layer_counts[c]; ++l) {
      const double thick = thicknesses[c * COATING_MAX_LAYERS + l];
      if (!(thick >= 0.0 && thick < PRT_INF)) return fail(PRT_ERR_ARG, "coatings: thicknesses finite and >= 0");
    }
    args.n_layers[c] = layer_counts[c];
    args.has_substrate[c] = has_substrate[c] != 0;
  }
  for (int s = 0; s < n_coated; ++s) {
    if (surface_coating[s] < 0 || surface_coating[s] >= n_coatings)
      return fail(PRT_ERR_ARG, "coatings: a surface names a coating that is not there");
    for (int r = 0; r < s; ++r)
      if (coated_surfaces[r] == coated_surfaces[s]) return fail(PRT_ERR_ARG, "coatings: a surface is listed twice");
    for (int r = 0; r < n_lossless; ++r)
      if (lossless[r] == coated_surfaces[s]) return fail(PRT_ERR_ARG, "coatings: a surface is both lossless and coated");
    args.coated[s] = (double)coated_surfaces[s];
    args.coating_of[s] = surface_coating[s];
  }
  args.n_lossless = n_lossless;
  args.n_coated = n_coated;
  args.n_wavelengths = n_wavelengths;
  for (int k = 0; k < n_lossless; ++k) args.lossless[k] = (double)lossless[k];
  if (polarization) {
    const double x = polarization[0], y = polarization[1], z = polarization[2];
    const double a = polarization[3], b = polarization[4], c = polarization[5];
    const double m = std::sqrt(((x * x + y * y) + z * z) + ((a * a + b * b) + c * c));
    if (!(m > 0.0 && m < PRT_INF)) return fail(PRT_ERR_ARG, "fresnel: polarization finite and not zero");
    args.polarised = 1;
    args.vr[0] = x / m; args.vr[1] = y / m; args.vr[2] = z / m;
    args.vi[0] = a / m; args.vi[1] = b / m; args.vi[2] = c / m;
  }
  for (int k = 0; k < COATED_COUNTERS; ++k) record_out[k] = 0;
  if (n_rows == 0) return PRT_OK;
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_fresnel_coated_workspace_bytes)
  CoatedWords* words = (CoatedWords*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  double* d_thickness = (double*)((char*)words + 64);
  double* d_wavelengths = d_thickness + COATING_MAX_COATINGS * COATING_MAX_LAYERS;
  double* d_indices = d_wavelengths + COATING_MAX_WAVELENGTHS;
  double* field = (double*)((char*)d_thickness + kCoatedTableBytes);
  int64_t* last_row = (int64_t*)(field + 12 * n_ids);
  int* stamp = (int*)(last_row + n_ids);
  HIP_TRY(hipMemsetAsync(words, 0, 64, st));
  HIP_TRY(hipMemsetAsync(stamp, 0, (size_t)n_ids * sizeof(int), st));
  if (n_coatings) {
    HIP_TRY(hipMemcpyAsync(d_thickness, thicknesses, sizeof(double) * n_coatings * COATING_MAX_LAYERS,
                           hipMemcpyHostToDevice, st));
    if (n_wavelengths) {
      HIP_TRY(hipMemcpyAsync(d_wavelengths, wavelengths, sizeof(double) * n_wavelengths, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_indices, indices, sizeof(double) * 2 * n_coatings * COATING_SLOTS * n_wavelengths,
                             hipMemcpyHostToDevice, st));
    }
  }
  int64_t start = 0;
  for (int g = 0; g < n_generations; ++g) {
    const int64_t count = rows_per_generation[g];
    if (count)
      hipLaunchKernelGGL(k_coated_fresnel_step, dim3((unsigned)((count + kFresnelBlock - 1) / kFresnelBlock)),
                         dim3(kFresnelBlock), 0, st, rows, ld, n_rows, start, count, g, id0, n_ids, args, d_thickness,
                         d_wavelengths, d_indices, field, last_row, stamp, words, transmittance_out, field_out);
    start += count;
  }
  CoatedWords host_words;
  HIP_TRY(hipMemcpyAsync(&host_words, words, sizeof(CoatedWords), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  const int status = host_words.status;
  if (status & FRESNEL_BAD_ID) return fail(PRT_ERR_ARG, "fresnel: an id is not an integer in [id0, id0 + n_ids)");
  if (status & FRESNEL_REPEATED_ID) return fail(PRT_ERR_ARG, "fresnel: an id repeats within a generation");
  if (status & FRESNEL_NOT_WHOLE)
    return fail(PRT_ERR_ARG, "fresnel: a ray has a row in a generation and none in the one before: the frame is not whole");
  if (status & FRESNEL_NO_WAVELENGTH)
    return fail(PRT_ERR_ARG, "coatings: a row's wavelength at a coated surface is not in the table of wavelengths");
  for (int k = 0; k < COATED_COUNTERS; ++k) record_out[k] = (int64_t)host_words.count[k];
  return PRT_OK;
}

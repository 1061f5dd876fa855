// prt_fresnel.hpp -- Fresnel transmittance and polarisation of the frame, on the device: every
// ray's two field vectors carried through the interfaces its rows describe, and per row the share of its launch energy
// that is left.  It uses the join by ray id (prt_join.hpp) and has the optical path's shape: one launch per generation,
// one row a thread.  Definitions: include/prt.h.
//
//   fresnel_row      the work of one row, written once for both steps and parameterised on the field type: FrVec (real
//                    fields, six planes of state per id) here, CxVec (complex fields, twelve planes) with the coatings
//                    of prt_coatings.hpp, whose part lies behind `if constexpr`.  Per id: the stamp, the row it had in
//                    the previous generation, and Ea, Eb as planes of doubles, real parts first (lane i of a wave reads
//                    element i of every plane when the ids are in order).  A row of generation g >= 1 reads its own
//                    direction and index, those of the ray's previous row and that row's surface, decides the
//                    interface's kind, updates the fields and writes its transmittance.
//   k_fresnel_step   one launch per generation, in generation order on one stream: fresnel_row on real fields, then
//                    the counters
// The previous row's NUMBER is kept per id, not its direction and index: 8 bytes of state instead of 40, written once
// and read once; the five values are then read from the frame, where the rows of one generation lie in the order of
// their ids as often as the rows that ask for them do, so the reads coalesce as the state's would.  The previous row's
// transmittance is read from the output for the same reason.
// No two lanes touch one ray's state (ids do not repeat within a generation), there are no floating-point atomics and
// no floating-point sums across rays; the counters are integers, summed over the wave (ballots) and the workgroup
// (LDS) and added with one atomic per workgroup.  Every output is the same bits on every run and under any order of the
// rows inside a generation.  The library is built with -ffp-contract=off: every product and sum below is rounded on its
// own, in the order written, which tests/fresnel_reference.py follows operation for operation.
#pragma once

enum { FRESNEL_NO_WAVELENGTH = JOIN_OWN_BIT };  // (after the join's bits; set at coated surfaces only)
// counters: reflections, lossless, undeviated, invalid rays; with coatings also coated interfaces and those of total
// internal reflection
enum { FRESNEL_MAX_LOSSLESS = 64, FRESNEL_COUNTERS = 4, COATED_COUNTERS = 6 };
static const int kFresnelBlock = 256;
static const int kFresnelWaves = kFresnelBlock / 64;
#define PRT_FRESNEL_EPS_DIR 1e-12  // eps_dir of include/prt.h

struct FresnelWords { u64 count[COATED_COUNTERS]; int status; };  // (cleared together, read back together: 52 <= 64 bytes)
// v: the unit polarisation vector, real parts and (complex fields) imaginary parts
struct FresnelArgs { double v[6]; int polarised, n_lossless; double lossless[FRESNEL_MAX_LOSSLESS]; };
struct FrVec { double x, y, z; };
struct NoCoatings { struct Coefficients {}; };  // (what k_fresnel_step passes where the coated step passes its tables)

__device__ __forceinline__ double fr_dot(const FrVec& a, const FrVec& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ FrVec fr_cross(const FrVec& a, const FrVec& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ FrVec fr_over(const FrVec& a, double m) { return {a.x / m, a.y / m, a.z / m}; }
__device__ __forceinline__ FrVec fr_unit(const FrVec& a) { return fr_over(a, sqrt(fr_dot(a, a))); }
__device__ __forceinline__ FrVec fr_tilt(const double* __restrict__ rows, int64_t ld, int64_t j) {
  return {rows[PRT_COL_XTILT * ld + j], rows[PRT_COL_YTILT * ld + j], rows[PRT_COL_ZTILT * ld + j]};
}
// v - (v.u) u: the part of v across the unit vector u
__device__ __forceinline__ FrVec fr_across(const double* v, const FrVec& u) {
  const FrVec a = {v[0], v[1], v[2]};
  const double along = fr_dot(a, u);
  return {a.x - along * u.x, a.y - along * u.y, a.z - along * u.z};
}

// ---- what fresnel_row asks of a field vector; prt_coatings.hpp gives the same for CxVec, part by part ----------------------
__device__ __forceinline__ void fr_fill(FrVec& e, double c) { e = {c, c, c}; }
__device__ __forceinline__ void fr_real(FrVec& e, const FrVec& r) { e = r; }
// element i of three planes of doubles that lie n apart (Ea from `planes`, Eb from planes + 3 n)
__device__ __forceinline__ void fr_load(FrVec& e, const double* planes, int64_t n, int64_t i) {
  e = {planes[i], planes[n + i], planes[2 * n + i]};
}
__device__ __forceinline__ void fr_store(const FrVec& e, double* planes, int64_t n, int64_t i) {
  planes[i] = e.x; planes[n + i] = e.y; planes[2 * n + i] = e.z;
}
__device__ __forceinline__ FrVec fr_scale(const FrVec& e, double c) { return {c * e.x, c * e.y, c * e.z}; }
// E' = (cs (E.s)) s + (cp (E.pi)) pt
__device__ __forceinline__ FrVec fr_through(const FrVec& e, const FrVec& s, const FrVec& pi, const FrVec& pt, double cs,
                                            double cp) {
  const double fs = cs * fr_dot(e, s), fp = cp * fr_dot(e, pi);
  return {fs * s.x + fp * pt.x, fs * s.y + fp * pt.y, fs * s.z + fp * pt.z};
}
__device__ __forceinline__ double fr_norm2(const FrVec& e) { return fr_dot(e, e); }
// the launch field of a polarised ray along ut: v's part across ut, normalised; false when there is none
__device__ __forceinline__ bool fr_polarised(FrVec& e, const double* v, const FrVec& ut) {
  const FrVec w = fr_across(v, ut);
  const double ww = fr_dot(w, w);
  e = fr_over(w, sqrt(ww));
  return ww > PRT_FRESNEL_EPS_DIR;
}

// row j of `generation`; flag: what the row adds to the counters
template <class V, class Coatings, int N>
__device__ __forceinline__ void fresnel_row(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t j,
                                            int generation, double id0, int64_t n_ids, const FresnelArgs& args,
                                            const Coatings& coatings, double* __restrict__ field,
                                            int64_t* __restrict__ last_row, int* __restrict__ stamp, int* status,
                                            double* __restrict__ t_out, double* __restrict__ field_out, bool (&flag)[N]) {
  constexpr bool with_coatings = !std::is_same<Coatings, NoCoatings>::value;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  bool reflection = false, lossless = false, undeviated = false, invalid = false, coated = false, tir = false;
  V ea, eb;
  fr_fill(ea, nan);
  eb = ea;
  double t = nan;
  const int64_t i = join_id(rows, ld, j, id0, n_ids);
  bool joined = false, dead = true;
  if (i < 0) {
    atomicOr(status, JOIN_BAD_ID);
  } else {
    const int bits = join_status(join_claim(stamp, i, generation), generation);
    joined = !bits;
    if (bits) atomicOr(status, bits);
  }
  if (joined) {
    const FrVec raw = fr_tilt(rows, ld, j);
    const double mm = fr_dot(raw, raw);
    const FrVec ut = fr_over(raw, sqrt(mm));
    if (generation == 0) {
      invalid = !(mm > 0.0 && mm < PRT_INF);
      if (!invalid && args.polarised) {
        invalid = !fr_polarised(ea, args.v, ut);
        fr_fill(eb, 0.0);
      } else if (!invalid) {
        const double ax = fabs(ut.x), ay = fabs(ut.y), az = fabs(ut.z);
        int axis = 0;
        double least = ax;
        if (ay < least) { axis = 1; least = ay; }
        if (az < least) axis = 2;
        const FrVec e = {axis == 0 ? 1.0 : 0.0, axis == 1 ? 1.0 : 0.0, axis == 2 ? 1.0 : 0.0};
        const FrVec a = fr_unit(fr_cross(ut, e));
        fr_real(ea, a);
        fr_real(eb, fr_cross(ut, a));
      }
      t = 1.0;
      dead = invalid;
    } else {
      int64_t p = last_row[i];  // (written by the launch of generation - 1: the stamp said so)
      p = p >= 0 && p < n_rows ? p : j;
      const double t_before = t_out[p];
      // the ray's fields: with the rows' loads, but in the coated step after its layer loop, which needs the registers
      const auto load = [&] {
        fr_load(ea, field, n_ids, i);
        fr_load(eb, field + 3 * n_ids, n_ids, i);
      };
      if constexpr (!with_coatings) load();
      const FrVec ui = fr_unit(fr_tilt(rows, ld, p));
      const double ni = rows[PRT_COL_INDEX * ld + p], nt = rows[PRT_COL_INDEX * ld + j];
      const double surface = rows[PRT_COL_SURFACE * ld + p];
      for (int s = 0; s < args.n_lossless; ++s) lossless = lossless || surface == args.lossless[s];
      const FrVec d = {ui.x - ut.x, ui.y - ut.y, ui.z - ut.z};
      const double dd = fr_dot(d, d);
      t = t_before;
      if (!(dd < PRT_INF && ni > 0.0 && ni < PRT_INF && nt > 0.0 && nt < PRT_INF)) {
        invalid = true;  // (the fields: NaN as they stand)
      } else if (ni == nt && dd <= PRT_FRESNEL_EPS_DIR) {
        undeviated = true;
        if constexpr (with_coatings) load();
      } else {
        FrVec n;
        double ci, cs = -1.0, cp = 1.0;
        // from_fields: T follows from the fields (coefficients of magnitude 1 hand it on as it is: a rotation keeps |E|
        // only to rounding); by_stack: the coefficients are the stack's; refused: the fields pass, the call fails
        bool from_fields = false, by_stack = false, refused = false;
        [[maybe_unused]] typename Coatings::Coefficients z = {};
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
        if constexpr (with_coatings) {
          const int coating = coat_of(coatings, surface);
          if (coating >= 0) {  // (r, t of the stack instead; a coated interface never hands the transmittance on)
            coated = true;
            from_fields = true;
            z = coat_stack(coatings, coating, rows[PRT_COL_WAVELENGTH * ld + p], ni, nt, ci, xx, reflection);
            if (!z.found && !z.invalid) atomicOr(status, FRESNEL_NO_WAVELENGTH);
            invalid = invalid || z.invalid;
            by_stack = z.found;
            refused = !z.found && !invalid;
            tir = z.tir;
          }
          load();
        }
        // the interface applied to a field vector: with the stack's complex coefficients or with cs, cp
        const auto scaled = [&](const V& e) -> V {
          if constexpr (with_coatings)
            if (by_stack) return coat_times(e, z.zs);
          return fr_scale(e, cs);
        };
        const auto through = [&](const V& e, const FrVec& s, const FrVec& pi, const FrVec& pt) -> V {
          if constexpr (with_coatings)
            if (by_stack) return coat_through(e, s, pi, pt, z.zs, z.zp);
          return fr_through(e, s, pi, pt, cs, cp);
        };
        if (!refused) {
          if (xx <= PRT_FRESNEL_EPS_DIR) {  // (normal incidence: s and p coincide)
            ea = scaled(ea);
            eb = scaled(eb);
          } else {
            const FrVec s = fr_over(x, sqrt(xx)), pi = fr_cross(ui, s), pt = fr_cross(ut, s);
            ea = through(ea, s, pi, pt);
            eb = through(eb, s, pi, pt);
          }
          if (from_fields) {
            const double aa = fr_norm2(ea);
            t = args.polarised ? aa : (aa + fr_norm2(eb)) / 2.0;
          }
        }
      }
      dead = invalid || t_before != t_before;
      invalid = invalid && t_before == t_before;  // (a ray is counted once: it is NaN from there on)
    }
  }
  if (dead) {
    fr_fill(ea, nan);
    eb = ea;
    t = nan;
  }
  if (i >= 0) {  // (also for a row the status word refuses: what the next generation reads is this launch's own)
    fr_store(ea, field, n_ids, i);
    fr_store(eb, field + 3 * n_ids, n_ids, i);
    last_row[i] = j;
  }
  t_out[j] = t;
  if (field_out) {
    fr_store(ea, field_out, n_rows, j);
    fr_store(eb, field_out + 3 * n_rows, n_rows, j);
  }
  flag[0] = reflection; flag[1] = lossless; flag[2] = undeviated; flag[3] = invalid;
  if constexpr (with_coatings) { flag[4] = coated; flag[5] = tir; }
}

// the counters: over the wave, over the workgroup, one atomic each (every lane of the workgroup comes here)
template <int N>
__device__ __forceinline__ void fresnel_count(const bool (&flag)[N], u64* __restrict__ count) {
  __shared__ unsigned red[N][kFresnelWaves];
  unsigned tally[N];
#pragma unroll
  for (int c = 0; c < N; ++c) tally[c] = (unsigned)__popcll(__ballot(flag[c]));
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < N; ++c) red[c][threadIdx.x >> 6] = tally[c];
  __syncthreads();
  if (threadIdx.x < N) {
    unsigned sum = 0;
    for (int w = 0; w < kFresnelWaves; ++w) sum += red[threadIdx.x][w];
    if (sum) atomicAdd(count + threadIdx.x, (u64)sum);
  }
}

__global__ void __launch_bounds__(kFresnelBlock)
k_fresnel_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count, int generation,
               double id0, int64_t n_ids, FresnelArgs args, double* __restrict__ field, int64_t* __restrict__ last_row,
               int* __restrict__ stamp, FresnelWords* __restrict__ words, double* __restrict__ t_out,
               double* __restrict__ field_out) {
  const int64_t j = start + (int64_t)blockIdx.x * kFresnelBlock + threadIdx.x;
  bool flag[FRESNEL_COUNTERS] = {};
  if (j < start + count)
    fresnel_row<FrVec>(rows, ld, n_rows, j, generation, id0, n_ids, args, NoCoatings{}, field, last_row, stamp,
                       &words->status, t_out, field_out, flag);
  fresnel_count(flag, words->count);
}

// ---- entry points: what prt_frame_fresnel and prt_frame_fresnel_coated share -------------------------------------------
// the arguments the two have in common
struct FresnelCall {
  const double* rows; int64_t ld; const int64_t* rows_per_generation; int n_generations; double id0; int64_t n_ids;
  const double* polarization; const int64_t* lossless; int n_lossless; double* transmittance_out; int64_t* record_out;
  void *workspace, *stream;
};
struct FresnelWork { FresnelWords* words; char* tables; double* field; int64_t* last_row; int* stamp; };

// the words; the coated step's tables; per id: Ea and Eb (`planes` planes of doubles), its previous row, the stamp
static int64_t fresnel_workspace_bytes(int64_t n_rows, int64_t n_ids, int64_t table_bytes, int planes) {
  if (n_rows < 0 || !join_n_ids_ok(n_ids)) return PRT_ERR_ARG;
  return 64 + table_bytes + n_ids * (int64_t)(planes * sizeof(double) + sizeof(int64_t) + sizeof(int)) + 64;
}

static FresnelWork fresnel_carve(void* workspace, int64_t n_ids, int64_t table_bytes, int planes) {
  FresnelWork w;
  w.words = (FresnelWords*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  w.tables = (char*)w.words + 64;
  w.field = (double*)(w.tables + table_bytes);
  w.last_row = (int64_t*)(w.field + planes * n_ids);
  w.stamp = (int*)(w.last_row + n_ids);
  return w;
}

// Everything is checked before a device is touched, in this order: the buffers, the ids, the lossless surfaces, what
// `check_tables()` checks (the coated entry's tables), the polarisation (`parts` vectors: real, imaginary).  Fills
// args, clears the `counters` of record_out and returns the number of rows, or an error
template <class CheckTables>
static int64_t fresnel_check(const FresnelCall& c, int parts, int counters, FresnelArgs& args, CheckTables check_tables) {
  const int64_t n_rows = join_rows(c.rows_per_generation, c.n_generations, c.ld, kFresnelBlock, "fresnel");
  if (n_rows < 0) return n_rows;
  if (!c.record_out || !c.workspace || (n_rows && (!c.rows || !c.transmittance_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  int rc = join_ids(c.id0, c.n_ids);
  if (rc) return rc;
  if (c.n_lossless < 0 || c.n_lossless > FRESNEL_MAX_LOSSLESS || (c.n_lossless && !c.lossless))
    return fail(PRT_ERR_ARG, "fresnel: at most 64 lossless surfaces");
  std::memset(&args, 0, sizeof(args));
  args.n_lossless = c.n_lossless;
  for (int k = 0; k < c.n_lossless; ++k) args.lossless[k] = (double)c.lossless[k];
  rc = check_tables();
  if (rc) return rc;
  if (c.polarization) {
    double sum = 0.0;  // ((x x + y y) + z z of the real parts, then + the same of the imaginary parts)
    for (const double* v = c.polarization; v < c.polarization + 3 * parts; v += 3)
      sum += (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double m = std::sqrt(sum);
    if (!(m > 0.0 && m < PRT_INF)) return fail(PRT_ERR_ARG, "fresnel: polarization finite and not zero");
    args.polarised = 1;
    for (int k = 0; k < 3 * parts; ++k) args.v[k] = c.polarization[k] / m;
  }
  for (int k = 0; k < counters; ++k) c.record_out[k] = 0;
  return n_rows;
}

// the launches, one per generation in order (`launch(grid, start, count, generation)`), and what they report
template <class Launch>
static int fresnel_run(const FresnelCall& c, int64_t n_rows, const FresnelWork& w, int counters, Launch launch) {
  hipStream_t st = (hipStream_t)c.stream;
  HIP_TRY(hipMemsetAsync(w.words, 0, 64, st));
  HIP_TRY(hipMemsetAsync(w.stamp, 0, (size_t)c.n_ids * sizeof(int), st));
  int64_t start = 0;
  for (int g = 0; g < c.n_generations; ++g) {
    const int64_t count = c.rows_per_generation[g];
    if (count) launch(dim3((unsigned)((count + kFresnelBlock - 1) / kFresnelBlock)), start, count, g);
    start += count;
  }
  FresnelWords host_words;
  HIP_TRY(hipMemcpyAsync(&host_words, w.words, sizeof(FresnelWords), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  const int rc = join_refusal(host_words.status, "fresnel");
  if (rc) return rc;
  if (host_words.status & FRESNEL_NO_WAVELENGTH)
    return fail(PRT_ERR_ARG, "coatings: a row's wavelength at a coated surface is not in the table of wavelengths");
  for (int k = 0; k < counters; ++k) c.record_out[k] = (int64_t)host_words.count[k];
  return PRT_OK;
}

extern "C" int64_t prt_frame_fresnel_workspace_bytes(int64_t n_rows, int64_t n_ids) {
  return fresnel_workspace_bytes(n_rows, n_ids, 0, 6);
}

extern "C" int prt_frame_fresnel(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                 int n_generations, double id0, int64_t n_ids, const double* polarization,
                                 const int64_t* lossless, int n_lossless, double* transmittance_out, double* field_out,
                                 int64_t* record_out, void* workspace, void* stream) {
  const FresnelCall c = {rows, ld, rows_per_generation, n_generations, id0, n_ids, polarization, lossless, n_lossless,
                         transmittance_out, record_out, workspace, stream};
  FresnelArgs args;
  const int64_t n_rows = fresnel_check(c, 1, FRESNEL_COUNTERS, args, [] { return PRT_OK; });
  if (n_rows <= 0) return (int)n_rows;
  int rc = ops_device(device);
  if (rc) return rc;
  const FresnelWork w = fresnel_carve(workspace, n_ids, 0, 6);
  return fresnel_run(c, n_rows, w, FRESNEL_COUNTERS, [&](dim3 grid, int64_t start, int64_t count, int g) {
    hipLaunchKernelGGL(k_fresnel_step, grid, dim3(kFresnelBlock), 0, (hipStream_t)stream, rows, ld, n_rows, start, count, g,
                       id0, n_ids, args, w.field, w.last_row, w.stamp, w.words, transmittance_out, field_out);
  });
}

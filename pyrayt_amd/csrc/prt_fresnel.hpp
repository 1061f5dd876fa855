// prt_fresnel.hpp -- Fresnel transmittance and polarisation of the frame, on the device: every
// ray's two field vectors carried through the interfaces its rows describe, and per row the share of its launch energy
// that is left.  It is the fourth use of the join by ray id (k_frame_optical_path, k_aberration_table, k_paths_step)
// and has the optical path's shape: one launch per generation, one row a thread.  Definitions: include/prt.h.
//
//   k_fresnel_step   one launch per generation, in generation order on one stream.  Per id: the generation that wrote it
//                    last + 1 (an atomic exchange, which also finds a repeated id and a missing generation), the row it
//                    had there, and Ea, Eb as six planes of doubles (lane i of a wave reads element i of every plane
//                    when the ids are in order).  A row of generation g >= 1 reads its own direction and index, those
//                    of the ray's previous row and that row's surface, decides the interface's kind, updates the
//                    fields and writes its transmittance.
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

enum { FRESNEL_BAD_ID = 1, FRESNEL_REPEATED_ID = 2, FRESNEL_NOT_WHOLE = 4 };
enum { FRESNEL_MAX_LOSSLESS = 64, FRESNEL_COUNTERS = 4 };  // counters: reflections, lossless, undeviated, invalid rays
static const int kFresnelBlock = 256;
static const int kFresnelWaves = kFresnelBlock / 64;
#define PRT_FRESNEL_EPS_DIR 1e-12  // eps_dir of include/prt.h

struct FresnelWords { u64 count[FRESNEL_COUNTERS]; int status; };       // (cleared together, read back together)
struct FresnelArgs { double v[3]; int polarised, n_lossless; double lossless[FRESNEL_MAX_LOSSLESS]; };
struct FrVec { double x, y, z; };

__device__ __forceinline__ double fr_dot(const FrVec& a, const FrVec& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ FrVec fr_cross(const FrVec& a, const FrVec& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ FrVec fr_over(const FrVec& a, double m) { return {a.x / m, a.y / m, a.z / m}; }
__device__ __forceinline__ FrVec fr_unit(const FrVec& a) { return fr_over(a, sqrt(fr_dot(a, a))); }
__device__ __forceinline__ FrVec fr_tilt(const double* __restrict__ rows, int64_t ld, int64_t j) {
  return {rows[PRT_COL_XTILT * ld + j], rows[PRT_COL_YTILT * ld + j], rows[PRT_COL_ZTILT * ld + j]};
}
// E' = (cs (E.s)) s + (cp (E.pi)) pt
__device__ __forceinline__ FrVec fr_through(const FrVec& e, const FrVec& s, const FrVec& pi, const FrVec& pt, double cs,
                                            double cp) {
  const double fs = cs * fr_dot(e, s), fp = cp * fr_dot(e, pi);
  return {fs * s.x + fp * pt.x, fs * s.y + fp * pt.y, fs * s.z + fp * pt.z};
}

__global__ void __launch_bounds__(kFresnelBlock)
k_fresnel_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count, int generation,
               double id0, int64_t n_ids, FresnelArgs args, double* __restrict__ field, int64_t* __restrict__ last_row,
               int* __restrict__ stamp, FresnelWords* __restrict__ words, double* __restrict__ t_out,
               double* __restrict__ field_out) {
  __shared__ unsigned red[FRESNEL_COUNTERS][kFresnelWaves];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t j = start + (int64_t)blockIdx.x * kFresnelBlock + threadIdx.x;
  bool reflection = false, lossless = false, undeviated = false, invalid = false;
  if (j < start + count) {
    FrVec ea = {nan, nan, nan}, eb = ea;
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
          const FrVec v = {args.v[0], args.v[1], args.v[2]};
          const double along = fr_dot(v, ut);
          const FrVec w = {v.x - along * ut.x, v.y - along * ut.y, v.z - along * ut.z};
          const double ww = fr_dot(w, w);
          invalid = !(ww > PRT_FRESNEL_EPS_DIR);
          ea = fr_over(w, sqrt(ww));
          eb = {0.0, 0.0, 0.0};
        } else if (!invalid) {
          const double ax = fabs(ut.x), ay = fabs(ut.y), az = fabs(ut.z);
          int axis = 0;
          double least = ax;
          if (ay < least) { axis = 1; least = ay; }
          if (az < least) axis = 2;
          const FrVec e = {axis == 0 ? 1.0 : 0.0, axis == 1 ? 1.0 : 0.0, axis == 2 ? 1.0 : 0.0};
          ea = fr_unit(fr_cross(ut, e));
          eb = fr_cross(ut, ea);
        }
        t = 1.0;
        dead = invalid;
      } else {
        int64_t p = last_row[i];  // (written by the launch of generation - 1: the stamp said so)
        p = p >= 0 && p < n_rows ? p : j;
        const double t_before = t_out[p];
        ea = {field[i], field[n_ids + i], field[2 * n_ids + i]};
        eb = {field[3 * n_ids + i], field[4 * n_ids + i], field[5 * n_ids + i]};
        const FrVec ui = fr_unit(fr_tilt(rows, ld, p));
        const double ni = rows[PRT_COL_INDEX * ld + p], nt = rows[PRT_COL_INDEX * ld + j];
        const double surface = rows[PRT_COL_SURFACE * ld + p];
        for (int s = 0; s < args.n_lossless; ++s) lossless = lossless || surface == args.lossless[s];
        const FrVec d = {ui.x - ut.x, ui.y - ut.y, ui.z - ut.z};
        const double dd = fr_dot(d, d);
        t = t_before;
        if (!(dd < PRT_INF && ni > 0.0 && ni < PRT_INF && nt > 0.0 && nt < PRT_INF)) {
          invalid = true;
        } else if (ni == nt && dd <= PRT_FRESNEL_EPS_DIR) {
          undeviated = true;
        } else {
          FrVec n;
          double cs = -1.0, cp = 1.0;
          reflection = ni == nt;
          if (reflection) {
            n = fr_over(d, sqrt(dd));
          } else {
            n = fr_unit({ni * ui.x - nt * ut.x, ni * ui.y - nt * ut.y, ni * ui.z - nt * ut.z});
            double ci = fr_dot(ui, n);
            if (ci < 0.0) { n = {-n.x, -n.y, -n.z}; ci = -ci; }
            const double ct = fr_dot(ut, n);
            invalid = !(ci > 0.0 && ct > 0.0);
            const double a = ni * ci, b = nt * ct, c = nt * ci, e = ni * ct;
            const double twice = 2.0 * sqrt(a * b);
            cs = lossless ? 1.0 : twice / (a + b);
            cp = lossless ? 1.0 : twice / (c + e);
          }
          const FrVec x = fr_cross(ui, n);
          const double xx = fr_dot(x, x);
          if (xx <= PRT_FRESNEL_EPS_DIR) {  // (normal incidence: s and p coincide)
            ea = {cs * ea.x, cs * ea.y, cs * ea.z};
            eb = {cs * eb.x, cs * eb.y, cs * eb.z};
          } else {
            const FrVec s = fr_over(x, sqrt(xx)), pi = fr_cross(ui, s), pt = fr_cross(ut, s);
            ea = fr_through(ea, s, pi, pt, cs, cp);
            eb = fr_through(eb, s, pi, pt, cs, cp);
          }
          // (coefficients of magnitude 1 hand the transmittance on as it is: a rotation keeps |E| only to rounding)
          if (!reflection && !lossless) {
            const double aa = fr_dot(ea, ea);
            t = args.polarised ? aa : (aa + fr_dot(eb, eb)) / 2.0;
          }
        }
        dead = invalid || t_before != t_before;
        invalid = invalid && t_before == t_before;  // (a ray is counted once: it is NaN from there on)
      }
    }
    if (dead) {
      ea = {nan, nan, nan};
      eb = ea;
      t = nan;
    }
    if (i >= 0) {  // (also for a row the status word refuses: what the next generation reads is this launch's own)
      field[i] = ea.x; field[n_ids + i] = ea.y; field[2 * n_ids + i] = ea.z;
      field[3 * n_ids + i] = eb.x; field[4 * n_ids + i] = eb.y; field[5 * n_ids + i] = eb.z;
      last_row[i] = j;
    }
    t_out[j] = t;
    if (field_out) {
      field_out[j] = ea.x; field_out[n_rows + j] = ea.y; field_out[2 * n_rows + j] = ea.z;
      field_out[3 * n_rows + j] = eb.x; field_out[4 * n_rows + j] = eb.y; field_out[5 * n_rows + j] = eb.z;
    }
  }
  // the counters: over the wave, over the workgroup, one atomic each
  const unsigned tally[FRESNEL_COUNTERS] = {(unsigned)__popcll(__ballot(reflection)), (unsigned)__popcll(__ballot(lossless)),
                                            (unsigned)__popcll(__ballot(undeviated)), (unsigned)__popcll(__ballot(invalid))};
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < FRESNEL_COUNTERS; ++c) red[c][threadIdx.x >> 6] = tally[c];
  __syncthreads();
  if (threadIdx.x < FRESNEL_COUNTERS) {
    unsigned sum = 0;
    for (int w = 0; w < kFresnelWaves; ++w) sum += red[threadIdx.x][w];
    if (sum) atomicAdd(&words->count[threadIdx.x], (u64)sum);
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------
static bool fresnel_sizes_ok(int64_t n_rows, int64_t n_ids) {
  return n_rows >= 0 && n_ids >= 1 && n_ids <= ((int64_t)1 << 31);
}

extern "C" int64_t prt_frame_fresnel_workspace_bytes(int64_t n_rows, int64_t n_ids) {
  if (!fresnel_sizes_ok(n_rows, n_ids)) return PRT_ERR_ARG;
  // the words; per id: Ea and Eb (six planes of doubles), its previous row, the stamp
  return 64 + n_ids * (int64_t)(6 * sizeof(double) + sizeof(int64_t) + sizeof(int)) + 64;
}

extern "C" int prt_frame_fresnel(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                 int n_generations, double id0, int64_t n_ids, const double* polarization,
                                 const int64_t* lossless, int n_lossless, double* transmittance_out, double* field_out,
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
  FresnelArgs args;
  std::memset(&args, 0, sizeof(args));
  args.n_lossless = n_lossless;
  for (int k = 0; k < n_lossless; ++k) args.lossless[k] = (double)lossless[k];
  if (polarization) {
    const double x = polarization[0], y = polarization[1], z = polarization[2];
    const double m = std::sqrt((x * x + y * y) + z * z);
    if (!(m > 0.0 && m < PRT_INF)) return fail(PRT_ERR_ARG, "fresnel: polarization finite and not zero");
    args.polarised = 1;
    args.v[0] = x / m; args.v[1] = y / m; args.v[2] = z / m;
  }
  for (int k = 0; k < FRESNEL_COUNTERS; ++k) record_out[k] = 0;
  if (n_rows == 0) return PRT_OK;
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_fresnel_workspace_bytes)
  FresnelWords* words = (FresnelWords*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  double* field = (double*)((char*)words + 64);
  int64_t* last_row = (int64_t*)(field + 6 * n_ids);
  int* stamp = (int*)(last_row + n_ids);
  HIP_TRY(hipMemsetAsync(words, 0, 64, st));
  HIP_TRY(hipMemsetAsync(stamp, 0, (size_t)n_ids * sizeof(int), st));
  int64_t start = 0;
  for (int g = 0; g < n_generations; ++g) {
    const int64_t count = rows_per_generation[g];
    if (count)
      hipLaunchKernelGGL(k_fresnel_step, dim3((unsigned)((count + kFresnelBlock - 1) / kFresnelBlock)), dim3(kFresnelBlock),
                         0, st, rows, ld, n_rows, start, count, g, id0, n_ids, args, field, last_row, stamp, words,
                         transmittance_out, field_out);
    start += count;
  }
  FresnelWords host_words;
  HIP_TRY(hipMemcpyAsync(&host_words, words, sizeof(FresnelWords), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  const int status = host_words.status;
  if (status & FRESNEL_BAD_ID) return fail(PRT_ERR_ARG, "fresnel: an id is not an integer in [id0, id0 + n_ids)");
  if (status & FRESNEL_REPEATED_ID) return fail(PRT_ERR_ARG, "fresnel: an id repeats within a generation");
  if (status & FRESNEL_NOT_WHOLE)
    return fail(PRT_ERR_ARG, "fresnel: a ray has a row in a generation and none in the one before: the frame is not whole");
  for (int k = 0; k < FRESNEL_COUNTERS; ++k) record_out[k] = (int64_t)host_words.count[k];
  return PRT_OK;
}

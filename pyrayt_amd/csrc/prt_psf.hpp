// prt_psf.hpp -- the diffraction PSF (Huygens sum) and the Strehl ratio of the frame, on the device (DESIGN.md
// section 4.5).  It builds on prt_wavefront.hpp: the rows prt_frame_wavefront selected, its OPD, pupil points and group
// records.  Definitions: include/prt.h.
//
// The first part is the Huygens core that every diffraction pass stands on (this one, the polarised one and the
// sensitivities): on the host the wavelength list, the grid checks, the plan of the sort and of the slices, the scratch
// and the status word; on the device the wavelength of a row, the rule for keeping a ray, a wave's staged rays into
// their places (psf_place), a pixel's constants, the phase path and the fold of the Strehl slab.  The stable counting
// sort under it -- the runs of the row passes, the ballot loop, the scans, the tree -- is prt_sort.hpp's.
//
//   k_psf_count       per wave of a contiguous run of rows: how many rows the wavefront's filter selects
//   (k_sort_positions: the waves' output offsets, the order of the wavefront's opd_out / pupil_out)
//   k_psf_stage       per selected row, in row order: p1, p2, c = (OPD - R) s, a = sqrt(w) and its (group, wavelength)
//                     bucket; per wave and bucket the rays kept; rays left out counted per bucket (integer atomics)
//   (k_sort_offsets, k_sort_starts: each wave's offset inside each bucket, each bucket's total and start)
//   k_psf_scatter     the stable counting sort: every wave writes its rays, in order, at its offsets
//   k_psf_strehl      per (ray slice, bucket, quantity): sum a, sum a cos / sin (2 pi OPD s) in fp64, a fixed tree order;
//                     with K parameters, quantity 1 + k: sum a e_k cos / sin (here K = 0)
//   k_psf_record      per group: the slices folded in order, the record, the Strehl ratio and the normalisation
//   k_psf_huygens     per (pixel tile, ray slice, bucket): the complex amplitude sum of the slice's rays at every pixel
//                     of the tile, the rays walked through LDS; partial sums into a slab of its own
//   k_psf_fold        per (bucket, pixel): the slices added in slice order, |U|^2 / lambda_w^2, normalised
// No floating-point atomics: every output is the same, bit for bit, on every run.
#pragma once

enum { PSF_MAX_WAVELENGTHS = 16, PSF_MAX_SIDE = 1024, PSF_RECORD = 4, PSF_BAD_WAVELENGTH = 1 };
static const int kPsfBlock = 256;                 // threads of a Huygens workgroup = rays of its LDS tile
static const int kPsfPix = 4;                     // pixels a thread owns (fp64 complex accumulators in registers)
static const int kPsfTile = kPsfBlock * kPsfPix;  // pixels of a workgroup
static const int kPsfMinSlice = 2048;             // rays a slice should hold at least
static const int kPsfMaxSlices = 1024;
static const size_t kPsfSlabBytes = 256u << 20;   // cap on the (bucket, slice, pixel) partial sums
static const size_t kPsfCountBytes = 64u << 20;   // cap on the sort's (wave, bucket) counts

struct PsfRay { double p1, p2, c, a; };
struct PsfPar { double e, q1, q2; };  // a parameter's share of a ray: e_k = dphase_k s, q_k = dpoint_k rho s
struct PsfLambda { double value[PSF_MAX_WAVELENGTHS], s[PSF_MAX_WAVELENGTHS]; int n; };

// ---- the core, host side --------------------------------------------------------------------------------------------
// `name` is the entry point's prefix of its messages
static int psf_lambda(const char* name, const double* wavelengths_um, int n_wavelengths, double world_unit_um,
                      PsfLambda& lambda) {
  if (n_wavelengths < 1 || n_wavelengths > PSF_MAX_WAVELENGTHS)
    return fail(PRT_ERR_ARG, std::string(name) + ": 1 to 16 distinct wavelengths");
  if (!(world_unit_um > 0 && world_unit_um < PRT_INF)) return fail(PRT_ERR_ARG, "world_unit_um: finite and > 0");
  lambda.n = n_wavelengths;
  for (int k = 0; k < PSF_MAX_WAVELENGTHS; ++k) lambda.value[k] = lambda.s[k] = 0.0;
  for (int k = 0; k < n_wavelengths; ++k) {
    const double w = wavelengths_um[k];
    if (!(w > 0 && w < PRT_INF)) return fail(PRT_ERR_ARG, "wavelengths: finite and > 0");
    for (int q = 0; q < k; ++q)
      if (wavelengths_um[q] == w) return fail(PRT_ERR_ARG, "wavelengths: distinct");
    lambda.value[k] = w;
    lambda.s[k] = 1.0 / (w / world_unit_um);
    if (!(lambda.s[k] < PRT_INF)) return fail(PRT_ERR_ARG, "wavelengths: wavelength / world_unit_um underflows");
  }
  return PRT_OK;
}

static int psf_grid(const char* name, int nx, int ny, double du, double dv, const double* centre_uv) {
  const std::string at = std::string(name) + ": ";
  if (nx < 1 || nx > PSF_MAX_SIDE || ny < 1 || ny > PSF_MAX_SIDE) return fail(PRT_ERR_ARG, at + "nx, ny in 1..1024");
  if (!(du > 0 && du < PRT_INF && dv > 0 && dv < PRT_INF)) return fail(PRT_ERR_ARG, at + "du, dv finite and > 0");
  if (!(std::isfinite(centre_uv[0]) && std::isfinite(centre_uv[1]))) return fail(PRT_ERR_ARG, at + "centre finite");
  return PRT_OK;
}

// The sort walks n_items (all rows of the frame, or the selection) into sort_buckets (group, wavelength) buckets; the
// sums run per bucket of `buckets` (the polarised pass: a sort bucket per state) over npix pixels, tile_pixels a
// workgroup.  pixel_bytes: a pixel of the partial-sum slab as the slices are capped; stored_bytes: as it is allocated
// (the sensitivities cap for 16 parameters whatever K is, so that the slices do not follow K); strehl_sums: doubles
// per (bucket, slice).  The slice count decides the order of the slice fold, and with it the bits.
struct PsfPlan {
  int64_t per_wave, all_waves, tiles, slices;
  unsigned grid;
  size_t count_bytes, strehl_bytes, slab_bytes;
};
static PsfPlan psf_plan(int cus, int64_t n_items, int64_t sort_buckets, int64_t buckets, int64_t npix,
                        int64_t tile_pixels, size_t pixel_bytes, size_t stored_bytes, size_t strehl_sums) {
  PsfPlan p;
  // row passes: waves of contiguous rows, as many as the (wave, bucket) counts allow
  const SortPlan sort = sort_plan(n_items, sort_buckets, 8, kPsfCountBytes);
  p.per_wave = sort.per_wave, p.grid = sort.grid, p.all_waves = sort.all_waves, p.count_bytes = sort.count_bytes;
  // ray slices: enough workgroups to fill the CUs, slices of at least kPsfMinSlice items of an average sort bucket
  const int64_t tiles = (npix + tile_pixels - 1) / tile_pixels;
  int64_t slices = (4 * (int64_t)cus + tiles * buckets - 1) / (tiles * buckets);
  slices = std::min<int64_t>(slices, std::max<int64_t>(1, n_items / (sort_buckets * kPsfMinSlice)));
  slices = std::min<int64_t>(slices, (int64_t)(kPsfSlabBytes / ((size_t)buckets * npix * pixel_bytes)));
  slices = std::max<int64_t>(1, std::min<int64_t>(slices, kPsfMaxSlices));
  p.tiles = tiles;
  p.slices = slices;
  p.strehl_bytes = (size_t)buckets * slices * strehl_sums * sizeof(double);
  p.slab_bytes = (size_t)buckets * slices * npix * stored_bytes;
  return p;
}

// the device, its CU count, and the scratch of a plan: the sort's counts zeroed, and `zeroed` (the workspace's counters
// of rays left out, with the status word behind them)
struct PsfScratch { char* base; int64_t* counts; double *strehl_slab, *slab; };
static int psf_device(int device, int* cus) {
  const int rc = ops_device(device);
  return rc ? rc : hist_cus(device, cus);
}
static int psf_scratch(hipStream_t st, const PsfPlan& p, void* zeroed, size_t zeroed_bytes, PsfScratch& s) {
  s.base = nullptr;
  HIP_TRY(hipMallocAsync((void**)&s.base, p.count_bytes + p.strehl_bytes + p.slab_bytes, st));
  s.counts = (int64_t*)s.base;
  s.strehl_slab = (double*)(s.base + p.count_bytes);
  s.slab = (double*)(s.base + p.count_bytes + p.strehl_bytes);
  HIP_TRY(hipMemsetAsync(s.counts, 0, p.count_bytes, st));
  HIP_TRY(hipMemsetAsync(zeroed, 0, zeroed_bytes, st));
  return PRT_OK;
}

// after the last launch: the status word read back, the scratch freed, the stream drained
static int psf_finish(hipStream_t st, const int* status, const PsfScratch& s, int* host_status) {
  *host_status = 0;
  HIP_TRY(hipMemcpyAsync(host_status, status, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipFreeAsync(s.base, st));
  HIP_TRY(hipStreamSynchronize(st));  // (a caller's host arrays outlive their copies)
  HIP_TRY(hipGetLastError());
  return PRT_OK;
}

// ---- the core, device side ------------------------------------------------------------------------------------------
// the place of a row's wavelength in the list, -1 if it is not there
__device__ __forceinline__ int psf_wavelength(const PsfLambda& lambda, double wavelength) {
  int k = -1;
  for (int q = 0; q < lambda.n; ++q)
    if (k < 0 && lambda.value[q] == wavelength) k = q;
  return k;
}

// a ray is summed if its OPD and pupil point are numbers and its weight is finite and not negative
__device__ __forceinline__ bool psf_keep(double o, double x, double y, double w) {
  return o == o && x == x && y == y && w >= 0.0 && w < PRT_INF;
}

// a wave's staged rays [from, to): move(r, pos) for every ray r kept, pos its place in the sorted rays (sort_place)
template <class Move>
__device__ __forceinline__ void psf_place(int64_t from, int64_t to, const int* __restrict__ bucket_of, int64_t* mine,
                                          const int64_t* __restrict__ bucket_start, Move move) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = from; base < to; base += 64) {
    const int64_t r = base + lane;
    sort_place(lane, r < to ? bucket_of[r] : -1, mine, bucket_start, [&](int64_t pos) { move(r, pos); });
  }
}

// the rays [lo, hi) of bucket b's slice
__device__ __forceinline__ void psf_slice(const int64_t* __restrict__ bucket_total,
                                          const int64_t* __restrict__ bucket_start, int b, int slice, int slices,
                                          int64_t& lo, int64_t& hi) {
  const int64_t n = bucket_total[b], per = (n + slices - 1) / slices;
  lo = bucket_start[b] + (int64_t)slice * per;
  hi = bucket_start[b] + n;
  if (lo + per < hi) hi = lo + per;
}

// pixel `pix` of the grid (past the grid: pixel 0, computed and not stored): its place (u, v) in the image plane.  What
// a kernel keeps of it it forms itself, mu = -2 u, mv = -2 v and k0 = R^2 + u^2 + v^2 with |x - E|^2 = mu p1 + mv p2 + k0:
// formed in here, the compiler orders the set-up otherwise and numbers the registers of the kernels' loops otherwise
__device__ __forceinline__ void psf_pixel(int64_t pix, int64_t npix, int nx, int ny, double du, double dv, double u0,
                                          double v0, double& u, double& v) {
  const int i = pix < npix ? (int)(pix / ny) : 0, j = pix < npix ? (int)(pix - (int64_t)(pix / ny) * ny) : 0;
  u = u0 + ((double)i - 0.5 * (nx - 1)) * du;
  v = v0 + ((double)j - 0.5 * (ny - 1)) * dv;
}

// sqrt in fp64 for an argument far from 0 and from the denormals (|x - E|^2 ~ R^2): the hardware's reciprocal square
// root refined by Goldschmidt's iteration, as the compiler's own expansion does without its scaling steps.  And
// 1 / sqrt(x) from the same reciprocal square root: h = 0.5 / sqrt(x) after its one Goldschmidt step, doubled, and one
// Newton step against the finished root (three instructions that go where the caller drops it)
__device__ __forceinline__ double psf_sqrt(double x, double& inverse) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  double d = fma(-g, g, x);
  g = fma(d, h, g);
  d = fma(-g, g, x);
  g = fma(d, h, g);
  const double i = h + h;
  inverse = fma(fma(-g, i, 1.0), i, i);
  return g;
}

// The phase path of a (ray, pixel): cos and sin of 2 pi (OPD + d - R) / lambda_w, and 1 / d
struct PsfPhase { double cs, sn, inverse; };
__device__ __forceinline__ PsfPhase psf_phase(double mu, double mv, double k0, double p1, double p2, double c,
                                              double s) {
  PsfPhase out;
  const double d2 = fma(mu, p1, fma(mv, p2, k0));      // |x - E|^2
  const double phase = fma(psf_sqrt(d2, out.inverse), s, c);     // (OPD + d - R) / lambda_w, cycles
  const float turn = (float)__builtin_amdgcn_fract(phase);       // [0, 1)
  out.cs = (double)__builtin_amdgcn_cosf(turn);                  // (v_cos_f32 / v_sin_f32 take turns)
  out.sn = (double)__builtin_amdgcn_sinf(turn);
  return out;
}

// the phase of a ray at P itself, for the Strehl sums: OPD / lambda_w in cycles, fp64 sincospi
__device__ __forceinline__ void psf_chief_phase(double radius, double s, double c, double& sn, double& cs) {
  const double phase = fma(radius, s, c);
  sincospi(2.0 * (phase - rint(phase)), &sn, &cs);
}

// strehl_slab: (bucket, slice, 1 + K, 3).  The slices of (bucket b, quantity) added in slice order
__device__ __forceinline__ void psf_strehl_fold(const double* __restrict__ strehl_slab, int slices, int K, int b,
                                                int quantity, double& a, double& c, double& s) {
  a = c = s = 0.0;
  for (int q = 0; q < slices; ++q) {
    const double* p = strehl_slab + (((size_t)b * slices + q) * (1 + K) + quantity) * 3;
    a += p[0]; c += p[1]; s += p[2];
  }
}

// ---- the kernels ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool psf_row(const double* __restrict__ rows, int64_t ld, int64_t j, double surface,
                                        double generation, double rays_per_source, int n_groups, int& group) {
  group = -1;
  if (wf_selected(rows, ld, j, surface, generation)) group = wf_group(rows, ld, j, rays_per_source, n_groups);
  return group >= 0;
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_psf_count(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface, double generation,
            double rays_per_source, int n_groups, int64_t per_wave, int64_t* __restrict__ wave_rows) {
  const auto [lane, wave, first, last] = sort_run(per_wave, n_rows);
  int64_t selected = 0;
  for (int64_t base = first; base < last; base += 64) {
    const int64_t j = base + lane;
    int group;
    selected += __popcll(__ballot(j < last && psf_row(rows, ld, j, surface, generation, rays_per_source, n_groups, group)));
  }
  if (lane == 0) wave_rows[wave] = selected;
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_psf_stage(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface, double generation,
            double rays_per_source, int n_groups, int64_t per_wave, const int64_t* __restrict__ wave_offset,
            const double* __restrict__ opd, const double* __restrict__ pupil, const double* __restrict__ group_record,
            int weight_column, PsfLambda lambda, PsfRay* __restrict__ stage, int* __restrict__ bucket_of,
            int64_t* __restrict__ counts, int buckets, unsigned long long* __restrict__ skipped,
            int* __restrict__ status) {
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
        if (psf_keep(o, x, y, w)) {
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
k_psf_scatter(const int64_t* __restrict__ wave_rows, const int64_t* __restrict__ wave_offset,
              const int* __restrict__ bucket_of, const PsfRay* __restrict__ stage, int64_t* __restrict__ offsets,
              const int64_t* __restrict__ bucket_start, int buckets, PsfRay* __restrict__ sorted) {
  const int64_t wave = sort_wave();
  const int64_t from = wave_offset[wave];  // (offsets + wave * buckets: only this wave reads and writes there)
  psf_place(from, from + wave_rows[wave], bucket_of, offsets + wave * buckets, bucket_start,
            [&](int64_t r, int64_t pos) { sorted[pos] = stage[r]; });
}

// strehl_slab: (bucket, slice, 1 + K, 3).  Quantity 0: sum a, sum a cos, sum a sin; quantity 1 + k: 0, sum a e_k cos,
// sum a e_k sin with e_k at par[k * n_items + ray] (no par where K is 0).  A group's record is group_ld doubles
__global__ void __launch_bounds__(kPsfBlock)
k_psf_strehl(const PsfRay* __restrict__ sorted, const PsfPar* __restrict__ par, int64_t n_items,
             const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
             const double* __restrict__ groups, PsfLambda lambda, int group_ld, int slices, int K,
             double* __restrict__ strehl_slab) {
  __shared__ double red[3][kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.x, b = blockIdx.y, quantity = blockIdx.z;
  const int g = b / lambda.n;
  const double s = lambda.s[b - g * lambda.n], radius = groups[(size_t)g * group_ld + 3];
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, b, slice, slices, lo, hi);
  double sum_a = 0.0, sum_c = 0.0, sum_s = 0.0;
  for (int64_t r = lo + t; r < hi; r += kPsfBlock) {
    const PsfRay ray = sorted[r];
    double sn, cs;
    psf_chief_phase(radius, s, ray.c, sn, cs);
    if (quantity == 0) {
      sum_a += ray.a;
      sum_c += ray.a * cs;
      sum_s += ray.a * sn;
    } else {
      const double ae = ray.a * par[(int64_t)(quantity - 1) * n_items + r].e;
      sum_c += ae * cs;
      sum_s += ae * sn;
    }
  }
  red[0][t] = sum_a; red[1][t] = sum_c; red[2][t] = sum_s;
  sort_tree(red, t);
  if (t < 3) strehl_slab[(((size_t)b * slices + slice) * (1 + K) + quantity) * 3 + t] = red[t][0];
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_psf_record(const double* __restrict__ strehl_slab, int slices, int n_groups, PsfLambda lambda,
             const int64_t* __restrict__ bucket_total, const unsigned long long* __restrict__ skipped,
             double* __restrict__ record_out, double* __restrict__ strehl_out, double* __restrict__ norm) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  double numerator = 0.0, denominator = 0.0;
  for (int k = 0; k < lambda.n; ++k) {
    const int b = g * lambda.n + k;
    double a, c, s;
    psf_strehl_fold(strehl_slab, slices, 0, b, 0, a, c, s);
    const double inv = lambda.s[k], num = inv * inv * (c * c + s * s), den = (inv * a) * (inv * a);
    double* o = record_out + (size_t)b * PSF_RECORD;
    o[0] = (double)bucket_total[b];
    o[1] = (double)skipped[b];
    o[2] = a;
    o[3] = num;
    numerator += num;
    denominator += den;
  }
  norm[g] = denominator;
  strehl_out[g] = denominator > 0.0 ? numerator / denominator : __longlong_as_double(0x7ff8000000000000ll);
}

__global__ void __launch_bounds__(kPsfBlock)
k_psf_huygens(const PsfRay* __restrict__ sorted, const int64_t* __restrict__ bucket_total,
              const int64_t* __restrict__ bucket_start, const double* __restrict__ group_record, PsfLambda lambda,
              int nx, int ny, double du, double dv, double u0, double v0, int slices, double* __restrict__ slab) {
  __shared__ PsfRay tile[kPsfBlock];
  const int t = threadIdx.x, slice = blockIdx.y, b = blockIdx.z;
  const int g = b / lambda.n;
  const double s = lambda.s[b - g * lambda.n], radius = group_record[(size_t)g * WF_GROUP + 3];
  const int64_t npix = (int64_t)nx * ny;
  double mu[kPsfPix], mv[kPsfPix], k0[kPsfPix], re[kPsfPix], im[kPsfPix];
#pragma unroll
  for (int q = 0; q < kPsfPix; ++q) {
    double u, v;
    psf_pixel((int64_t)blockIdx.x * kPsfTile + q * kPsfBlock + t, npix, nx, ny, du, dv, u0, v0, u, v);
    mu[q] = -2.0 * u;
    mv[q] = -2.0 * v;
    k0[q] = radius * radius + u * u + v * v;
    re[q] = im[q] = 0.0;
  }
  int64_t lo, hi;
  psf_slice(bucket_total, bucket_start, b, slice, slices, lo, hi);
  for (int64_t base = lo; base < hi; base += kPsfBlock) {
    __syncthreads();  // (the previous tile is read)
    if (base + t < hi) tile[t] = sorted[base + t];
    __syncthreads();
    const int count = hi - base < kPsfBlock ? (int)(hi - base) : kPsfBlock;
    for (int r = 0; r < count; ++r) {
      const PsfRay ray = tile[r];
#pragma unroll
      for (int q = 0; q < kPsfPix; ++q) {
        const PsfPhase at = psf_phase(mu[q], mv[q], k0[q], ray.p1, ray.p2, ray.c, s);
        re[q] = fma(ray.a, at.cs, re[q]);
        im[q] = fma(ray.a, at.sn, im[q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kPsfPix; ++q) {
    const int64_t pix = (int64_t)blockIdx.x * kPsfTile + q * kPsfBlock + t;
    if (pix < npix) {
      double* o = slab + (((size_t)b * slices + slice) * npix + pix) * 2;
      o[0] = re[q];
      o[1] = im[q];
    }
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_psf_fold(const double* __restrict__ slab, int slices, int buckets, int64_t npix, PsfLambda lambda,
           const double* __restrict__ norm, double* __restrict__ image_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)buckets * npix) return;
  const int b = (int)(item / npix);
  const int64_t pix = item - (int64_t)b * npix;
  double re = 0.0, im = 0.0;
  for (int q = 0; q < slices; ++q) {
    const double* p = slab + (((size_t)b * slices + q) * npix + pix) * 2;
    re += p[0];
    im += p[1];
  }
  const int g = b / lambda.n;
  const double inv = lambda.s[b - g * lambda.n];
  image_out[item] = inv * inv * (re * re + im * im) / norm[g];  // (a group without rays: 0 / 0, NaN)
}

// ---- entry points ---------------------------------------------------------------------------------------------------
static int64_t psf_buckets_bytes(int n_groups, int n_wavelengths) {
  return (int64_t)n_groups * n_wavelengths * 8;
}

extern "C" int64_t prt_frame_psf_workspace_bytes(int64_t n_rows, int n_groups, int n_wavelengths) {
  if (n_rows < 0 || n_groups < 1 || n_wavelengths < 1 || n_wavelengths > PSF_MAX_WAVELENGTHS) return PRT_ERR_ARG;
  // wave counts and offsets, bucket totals / starts / skips, the status word, the groups' normalisation, the staged
  // and the sorted rays, the rays' buckets
  return (int64_t)2 * kWfMaxWaves * 8 + 3 * psf_buckets_bytes(n_groups, n_wavelengths) + 8 + (int64_t)n_groups * 8 +
         n_rows * (int64_t)(2 * sizeof(PsfRay) + sizeof(int)) + 64;
}

extern "C" int prt_frame_psf(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                             double generation, double rays_per_source, int n_groups, const double* opd,
                             const double* pupil, const double* group_record, int weight_column,
                             const double* wavelengths_um, int n_wavelengths, double world_unit_um, int nx, int ny,
                             double du, double dv, const double* centre_uv, double* image_out, double* strehl_out,
                             double* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || n_groups < 1 || !group_record || !image_out || !strehl_out || !record_out ||
      !workspace || !wavelengths_um || !centre_uv || (n_rows && (!rows || !opd || !pupil)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  PsfLambda lambda;
  int rc = psf_lambda("psf", wavelengths_um, n_wavelengths, world_unit_um, lambda);
  if (!rc) rc = psf_grid("psf", nx, ny, du, dv, centre_uv);
  if (rc) return rc;
  const int64_t buckets = (int64_t)n_groups * n_wavelengths, npix = (int64_t)nx * ny;
  if (buckets > 65535) return fail(PRT_ERR_ARG, "psf: n_groups * n_wavelengths <= 65535");
  if ((size_t)buckets * npix * 2 * sizeof(double) > kPsfSlabBytes)
    return fail(PRT_ERR_ARG, "psf: n_groups * n_wavelengths * nx * ny * 16 bytes above the 256 MiB slab cap");
  int cus = 1;
  rc = psf_device(device, &cus);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_psf_workspace_bytes)
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
  const PsfPlan plan = psf_plan(cus, n_rows, buckets, buckets, npix, kPsfTile, 16, 16, 3);
  const int slices = (int)plan.slices, all_waves = (int)plan.all_waves;
  PsfScratch scratch;
  rc = psf_scratch(st, plan, skipped, (size_t)buckets * 8 + 8, scratch);  // (the skips and the status word)
  if (rc) return rc;
  hipLaunchKernelGGL(k_psf_count, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                     rays_per_source, n_groups, plan.per_wave, wave_rows);
  hipLaunchKernelGGL(k_sort_positions, dim3(1), dim3(kSortScanBlock), 0, st, all_waves, wave_rows, wave_offset);
  hipLaunchKernelGGL(k_psf_stage, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                     rays_per_source, n_groups, plan.per_wave, wave_offset, opd, pupil, group_record, weight_column,
                     lambda, stage, bucket_of, scratch.counts, (int)buckets, skipped, status);
  sort_offsets(st, all_waves, (int)buckets, scratch.counts, bucket_total, bucket_start);
  hipLaunchKernelGGL(k_psf_scatter, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, wave_rows, wave_offset, bucket_of, stage,
                     scratch.counts, bucket_start, (int)buckets, sorted);
  hipLaunchKernelGGL(k_psf_strehl, dim3((unsigned)slices, (unsigned)buckets), dim3(kPsfBlock), 0, st, sorted,
                     (const PsfPar*)nullptr, n_rows, bucket_total, bucket_start, group_record, lambda, (int)WF_GROUP,
                     slices, 0, scratch.strehl_slab);
  hipLaunchKernelGGL(k_psf_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     scratch.strehl_slab, slices, n_groups, lambda, bucket_total, skipped, record_out, strehl_out, norm);
  hipLaunchKernelGGL(k_psf_huygens, dim3((unsigned)plan.tiles, (unsigned)slices, (unsigned)buckets), dim3(kPsfBlock), 0,
                     st, sorted, bucket_total, bucket_start, group_record, lambda, nx, ny, du, dv, centre_uv[0],
                     centre_uv[1], slices, scratch.slab);
  hipLaunchKernelGGL(k_psf_fold, dim3((unsigned)((buckets * npix + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0,
                     st, scratch.slab, slices, (int)buckets, npix, lambda, norm, image_out);
  int host_status;
  rc = psf_finish(st, status, scratch, &host_status);
  if (rc) return rc;
  if (host_status & PSF_BAD_WAVELENGTH) return fail(PRT_ERR_ARG, "psf: a selected row's wavelength is not in the list");
  return PRT_OK;
}

// prt_sensitivity.hpp -- sensitivities of the frame, on the device: differential ray tracing.  A
// tangent (d position, d direction) per ray and parameter is pushed through the interfaces the ray's rows describe; out
// comes d(landing point)/d(parameter) of the selected rows and, per group, the sums a least-squares step needs.  It uses
// the join by ray id (prt_join.hpp) and has the Fresnel pass's shape: one launch per generation, one row a thread.
// Definitions: include/prt.h.
//
//   sens_row        the work of one row.  Per id: the stamp, the row it had in the previous generation (negative: the ray
//                   cannot be followed any more) and, per parameter, six planes of doubles: dx of the ray's last landing
//                   point and dd of the segment that ended there.  A row of generation g >= 1 reads its ray's previous
//                   row, finishes that row's interface (refraction, reflection, none), starts the new segment 1e-6 along
//                   the new direction and lands it on its own surface.  Everything that does not depend on the parameter
//                   (both normals, the curvature operator of the previous surface, the interface's kind) is worked out
//                   once, in registers; the loop over the parameters runs inside the thread with its state in memory, so
//                   the register count does not grow with K.  sens_row<true> is the design form (shape and index
//                   parameters): per parameter a 3x3 matrix S in the velocity u = v + w x (x - c) + S (x - c) and an index
//                   rate, each behind a bit, and a seventh plane of state, d(index of the ray's segment).  Its terms are
//                   added after the rigid ones, which are computed as in sens_row<false>: a parameter without the bits
//                   gets the bits of sens_row<false>.
//   k_sens_step     one launch per generation, in generation order on one stream: sens_row<false>, then the counters
//   k_sens_design_step  the same launch for sens_row<true>
//   k_sens_opd_step the design form plus an eighth plane, dL = d(cumulative optical path): sens_row<true, true>.  At a
//                   selected row it also writes the wavefront change per parameter (dfield, dopd, dpupil) against the fixed
//                   reference sphere of a wavefront pass, and the row's own OPD and pupil point
//   k_sens_launch_step, k_sens_launch_opd_step  the design and the wavefront form with the ray itself as a parameter:
//                   sens_row<true, false, true> and sens_row<true, true, true>.  A parameter may name rays (an id range) instead
//                   of surfaces: it seeds the tangent in generation 0 (a rigid motion of the launch) or feeds dnu from the
//                   dispersion of the Sellmeier glass the ray enters (a change of the wavelength); the step also writes dd of
//                   the selected rows (the slopes)
//   k_sens_partials the group sums of the selected rows as per-workgroup partials, written in workgroup order
//   k_sens_opd_partials  the wavefront sums (Z^T W y for K + 3 right-hand sides, the moments of dopd and dfield) as
//                   per-workgroup partials: a 64-row tile of factors in LDS, every entry a product of two of its columns
//   k_sens_fold     the partials of a group added in a fixed order: one wave per (group, entry)
// n, and the decision "wall or cap", come from the functions the trace uses: world_normal_len and object_normal of
// prt_device.hpp.  No two lanes touch one ray's state, there are no floating-point atomics; the sums run over the
// selection in the order the caller gave it (pyrayt_amd gives (group, generation, id)), so they do not depend on the
// order of the rows within a generation.  The library is built with -ffp-contract=off.
// Two things are not as the first design had them.  The surface table is NOT read through the scalar cache as the
// coating tables are: those are at most 64 entries in the kernel arguments, scanned by every lane alike; this table has
// no such cap (a system of a hundred lenses has three hundred surfaces) and the lanes of a wave meet different surfaces,
// so each lane bisects the table in the workspace and loads its own 200-byte entry with vector loads, which hit in the
// cache after the first wave.  And k_sens_partials keeps 206 x 4 doubles (6.5 KB) of LDS so that a workgroup needs one
// barrier for all its entries instead of two an entry; k_sens_step itself uses the 64 bytes of the counters and no more.
//
// The host side (from "entry points" down) has the Fresnel pass's shape.  The four entry points describe their call once
// -- SensCall, what all of them are given, and the parts a form adds: SensDesignCall, SensOpdCall, SensLaunchCall -- and
// which parts are present is the form.  sens_run is a sequence of steps with one job each:
//   sens_check      the buffers and sizes; gives n_rows and the rows of the largest group
//   sens_table      the surface table from the primitives
//   sens_rigid      the twists, and through sens_mark (the one bisection of the surface ids) the moved_by bits
//   sens_design     S, the index rates and the index_by bits
//   sens_launch     the seeds and the glass table
//   sens_layout     every pointer carved from the workspace, for every form; the four *_workspace_bytes functions are this
//                   layout from address 0
//   sens_upload, sens_steps (the form's step kernel, chosen once as a lambda), sens_sums, sens_report (the status words)
// Everything is refused before a device is touched, in the order of the steps.  The five __global__ step wrappers are
// written out one by one on purpose: profiles and kernel traces name them, and their arguments are their identity.
#pragma once

enum { SENS_BAD_SELECTION = JOIN_OWN_BIT };
enum { SENS_MAX_PARAMETERS = 16, SENS_MAX_IDS = 64, SENS_COUNTERS = 4, SENS_FIXED = 6 };
enum { SENS_MAX_ENTRIES = SENS_FIXED + 4 * SENS_MAX_PARAMETERS + SENS_MAX_PARAMETERS * (SENS_MAX_PARAMETERS + 1) / 2 };
static const int kSensBlock = 256;
static const int kSensWaves = kSensBlock / 64;
#define PRT_SENS_EPS_DIR 1e-12   // eps_dir of include/prt.h, as in the Fresnel pass
#define PRT_SENS_OFFSET 1e-6     // the relaunch offset

// a surface of the table: the fields of prt_prim that world_normal_len reads, and which parameters move it (bit k)
struct SensSurface {
  double minv[16];
  double params[6];
  double surface_id;
  int32_t type, normal_scale;
  uint32_t moved_by;
  uint32_t index_by;  // bit k: index parameter k names the surface (read by the design form alone)
};
struct SensTwist { double v[3], w[3], c[3]; };
struct SensArgs { SensTwist twist[SENS_MAX_PARAMETERS]; int n_parameters, n_surfaces; };
// the design form's own arguments: S (row-major, world) and the index rate per parameter; bit k of `linear` / `index`: the
// parameter has an S that is not zero / names surfaces whose index it changes
struct SensDesign { double S[SENS_MAX_PARAMETERS][9]; double rate[SENS_MAX_PARAMETERS]; uint32_t linear, index; };
// the launch form's own arguments: per parameter the ray ids [lo, hi) it names, as doubles, and the wavelength rate; bit k of
// `seeds` / `colour`: the parameter moves the launch of those rays (by its twist) / changes their wavelength
struct SensLaunch { double lo[SENS_MAX_PARAMETERS], hi[SENS_MAX_PARAMETERS], rate[SENS_MAX_PARAMETERS]; uint32_t seeds, colour; };
// the dispersion table: entry e is the material behind entry e of the surface table (SensSurface keeps its 200 bytes)
struct SensGlass { double coef[6]; int32_t kind, reserved; };
struct SensWords { u64 count[SENS_COUNTERS]; int status; };  // unknown, invalid, unfit, reflections
struct SensVec { double x, y, z; };
// the wavefront form's own arguments: the rows' cumulative optical path, per group (P (3), R, pivot, pupil radius), the
// device copy of group_first, the pupil basis, and the outputs in selection order
enum { SENS_OPD_GROUP = 6 };
struct SensOpd {
  const double* opl;
  const double* groups;
  const int64_t* first;
  int n_groups;
  double e1[3], e2[3];
  double *dfield, *dopd, *dpupil, *opd, *pupil;
};

__device__ __forceinline__ double sv_dot(const SensVec& a, const SensVec& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ SensVec sv_cross(const SensVec& a, const SensVec& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ SensVec sv_sub(const SensVec& a, const SensVec& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ SensVec sv_add(const SensVec& a, const SensVec& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ SensVec sv_scale(double c, const SensVec& a) { return {c * a.x, c * a.y, c * a.z}; }
__device__ __forceinline__ SensVec sv_col(const double* __restrict__ rows, int64_t ld, int first, int64_t j) {
  return {rows[first * ld + j], rows[(first + 1) * ld + j], rows[(first + 2) * ld + j]};
}
__device__ __forceinline__ bool sv_finite(const SensVec& a) { return is_finite(a.x) && is_finite(a.y) && is_finite(a.z); }

// the table's entry of a surface id (ascending ids), or -1
__device__ __forceinline__ int sens_find(const SensSurface* __restrict__ table, int n, double surface) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (table[mid].surface_id < surface) lo = mid + 1; else hi = mid;
  }
  return lo < n && table[lo].surface_id == surface ? lo : -1;
}

// A surface met at x by a ray along the unit vector d: n is the trace's world normal turned against d, nd = n.d < 0.
// The curvature operator dn = sign * (m - n (n.m)), m = A^T (h * (A y)) / denom for y = dx - u, is kept as h, sign
// and denom; h == 0 on flat pieces.
struct SensHit {
  SensVec n;
  double nd, sign, denom;
  int h;  // bit r: row r of A enters the Hessian (sphere 7, cylinder wall and paraboloid 3, flat 0)
  bool ok;
};

__device__ __forceinline__ SensHit sens_hit(const SensSurface* __restrict__ s, const SensVec& x, const SensVec& d) {
  SensHit hit;
  double len;
  world_normal_len(s, x.x, x.y, x.z, 1.0, hit.n.x, hit.n.y, hit.n.z, len);
  const double lx = row_dot(s->minv, 0, x.x, x.y, x.z, 1.0);
  const double ly = row_dot(s->minv, 1, x.x, x.y, x.z, 1.0);
  const double lz = row_dot(s->minv, 2, x.x, x.y, x.z, 1.0);
  double ax, ay, az;
  object_normal(s->type, s->params, lx, ly, lz, ax, ay, az);  // (wall or cap: what the trace decided)
  double g = 1.0;
  hit.h = 0;
  if (s->type == PRIM_SPHERE) {
    hit.h = 7;
    g = norm3(lx, ly, lz);
  } else if (s->type == PRIM_CYLINDER && az == 0.0) {
    hit.h = 3;
    g = norm3(lx, ly, 0.0);
  } else if (s->type == PRIM_PARABOLOID && az < 0.0) {
    hit.h = 3;
    g = norm3(lx, ly, 2 * s->params[0]);
  }
  hit.denom = len * g;
  hit.sign = (double)s->normal_scale;
  hit.nd = sv_dot(hit.n, d);
  if (hit.nd > 0.0) {
    hit.n = {-hit.n.x, -hit.n.y, -hit.n.z};
    hit.nd = -hit.nd;
    hit.sign = -hit.sign;
  }
  hit.ok = hit.nd < 0.0 && hit.nd >= -2.0 && (hit.h == 0 || (hit.denom > 0.0 && hit.denom < PRT_INF));
  return hit;
}

// the velocity of surface s under parameter k at x: v + w x (x - c) where k moves s, else 0
__device__ __forceinline__ SensVec sens_velocity(const SensTwist& tw, bool moved, const SensVec& x) {
  if (!moved) return {0.0, 0.0, 0.0};
  const SensVec r = {x.x - tw.c[0], x.y - tw.c[1], x.z - tw.c[2]};
  const SensVec w = {tw.w[0], tw.w[1], tw.w[2]};
  const SensVec t = sv_cross(w, r);
  return {tw.v[0] + t.x, tw.v[1] + t.y, tw.v[2] + t.z};
}

// S (x - c)
__device__ __forceinline__ SensVec sens_linear(const double* __restrict__ S, const SensTwist& tw, const SensVec& x) {
  const SensVec r = {x.x - tw.c[0], x.y - tw.c[1], x.z - tw.c[2]};
  return {(S[0] * r.x + S[1] * r.y) + S[2] * r.z, (S[3] * r.x + S[4] * r.y) + S[5] * r.z,
          (S[6] * r.x + S[7] * r.y) + S[8] * r.z};
}

enum { SENS_NONE = 0, SENS_REFRACT = 1, SENS_REFLECT = 2 };

// row j of `generation`; flag: what the row adds to the counters.  kDesign: `design` is read and the state has seven planes.
// kOpd (with kDesign): `wave` is read and the state has an eighth plane, dL; its terms come after everything else.
// kLaunch (with kDesign): `launch` and `glass` are read: a parameter may seed the tangent in generation 0 and may feed dnu
// from the dispersion of the glass the ray enters; dd of the selected rows goes to `slopes`.  Its terms sit behind the
// parameter's bits and the ray's id range, after everything else.
template <bool kDesign, bool kOpd = false, bool kLaunch = false>
__device__ __forceinline__ void sens_row(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t j,
                                         int generation, double id0, int64_t n_ids, const SensArgs& args,
                                         const SensSurface* __restrict__ table, double* __restrict__ state,
                                         int64_t* __restrict__ last_row, int* __restrict__ stamp, int* status,
                                         const int64_t* __restrict__ row_slot, int64_t n_selected,
                                         double* __restrict__ jacobian, bool (&flag)[SENS_COUNTERS],
                                         const SensDesign* design, const SensOpd* wave = nullptr,
                                         const SensLaunch* launch = nullptr, const SensGlass* __restrict__ glass = nullptr,
                                         double* __restrict__ slopes = nullptr) {
  constexpr int kPlanes = kOpd ? 8 : kDesign ? 7 : 6;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int K = args.n_parameters;
  bool unknown = false, invalid = false, unfit = false, reflection = false;
  int64_t slot = row_slot[j];
  if (slot >= n_selected) { atomicOr(status, SENS_BAD_SELECTION); slot = -1; }
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
    int64_t p = -1;
    bool was_dead = false;
    if (generation > 0) {
      p = last_row[i];  // (written by the launch of generation - 1: the stamp said so)
      was_dead = p < 0;
      p = was_dead ? -1 - p : p;
      p = p < n_rows ? p : j;
    }
    // this row: start, unit direction, landing point, surface
    const SensVec o = sv_col(rows, ld, PRT_COL_X0, j), x = sv_col(rows, ld, PRT_COL_X1, j);
    const SensVec raw = sv_col(rows, ld, PRT_COL_XTILT, j);
    const double mm = sv_dot(raw, raw);
    const SensVec d = sv_scale(1.0 / sqrt(mm), raw);
    const SensVec run = sv_sub(x, o);
    const double t = sv_dot(run, d);
    const int e = sens_find(table, args.n_surfaces, rows[PRT_COL_SURFACE * ld + j]);
    SensHit here = {};
    if (!(mm > 0.0 && mm < PRT_INF && sv_finite(o) && sv_finite(x))) {
      invalid = true;
    } else if (e < 0) {
      unknown = true;
    } else {
      here = sens_hit(table + e, x, d);
      invalid = !here.ok;
    }
    const uint32_t moved_here = e >= 0 ? table[e].moved_by : 0u;
    // the interface behind the previous row
    int kind = SENS_NONE;
    SensVec xp = {0, 0, 0}, dp = {0, 0, 0};
    SensHit there = {};
    double mu = 1.0, ci = 0.0, ct = 0.0, gamma = 0.0;
    double a0[3] = {0, 0, 0}, a1[3] = {0, 0, 0}, a2[3] = {0, 0, 0};
    uint32_t moved_there = 0u, index_there = 0u;
    double nt_there = 1.0;
    bool entering = false;
    double rid = 0.0, dndl = 0.0;  // (the launch form: the ray's id as the frame has it; dn/dlambda of the glass it enters)
    if constexpr (kLaunch) rid = rows[PRT_COL_ID * ld + j];
    if (generation > 0 && !was_dead && !invalid && !unknown) {
      xp = sv_col(rows, ld, PRT_COL_X1, p);
      const SensVec rawp = sv_col(rows, ld, PRT_COL_XTILT, p);
      dp = sv_scale(1.0 / sqrt(sv_dot(rawp, rawp)), rawp);
      const double ni = rows[PRT_COL_INDEX * ld + p], nt = rows[PRT_COL_INDEX * ld + j];
      const int ep = sens_find(table, args.n_surfaces, rows[PRT_COL_SURFACE * ld + p]);
      // (the previous row was landed by its own launch: its surface is in the table and its normal is good)
      if (ep < 0 || !(ni > 0.0 && ni < PRT_INF && nt > 0.0 && nt < PRT_INF)) {
        invalid = true;
      } else {
        const SensSurface* __restrict__ sp = table + ep;
        there = sens_hit(sp, xp, dp);
        moved_there = sp->moved_by;
        if constexpr (kDesign) {
          index_there = sp->index_by;
          nt_there = nt;
          entering = there.sign == (double)sp->normal_scale;  // (the trace's normal was not turned: refract4's !leaving)
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { a0[c] = sp->minv[c]; a1[c] = sp->minv[4 + c]; a2[c] = sp->minv[8 + c]; }
        const SensVec turn = sv_sub(dp, d);
        const double dd = sv_dot(turn, turn);
        ci = -there.nd;
        SensVec want;
        if (!there.ok || !(dd < PRT_INF)) {
          invalid = true;
          want = d;
        } else if (ni != nt) {
          kind = SENS_REFRACT;
          mu = ni / nt;
          const double radicand = 1.0 - (mu * mu) * (1.0 - ci * ci);
          ct = sqrt(radicand);
          gamma = mu * ci - ct;
          want = sv_add(sv_scale(mu, dp), sv_scale(gamma, there.n));
          unfit = !(radicand > 0.0);
        } else if (dd <= PRT_SENS_EPS_DIR) {
          want = d;
        } else {
          kind = SENS_REFLECT;
          reflection = true;
          want = sv_add(dp, sv_scale(2.0 * ci, there.n));
        }
        const SensVec miss = sv_sub(want, d);
        unfit = !invalid && (unfit || !(sv_dot(miss, miss) <= PRT_SENS_EPS_DIR));
        reflection = reflection && !unfit && !invalid;
        if constexpr (kLaunch) {  // Sellmeier: n^2 = 1 + sum b w^2 / (w^2 - c), dn/dlambda = -(sum b c w / (w^2 - c)^2) / n
          if (kind == SENS_REFRACT && entering && launch->colour && glass[ep].kind == MAT_SELLMEIER) {
            const double* __restrict__ q = glass[ep].coef;
            const double wl = rows[PRT_COL_WAVELENGTH * ld + j], w2 = wl * wl;
            const double t0 = w2 - q[3], t1 = w2 - q[4], t2 = w2 - q[5];
            const double n2 = ((1 + (q[0] * w2) / t0) + (q[1] * w2) / t1) + (q[2] * w2) / t2;
            const double down = (((q[0] * q[3]) * wl) / (t0 * t0) + ((q[1] * q[4]) * wl) / (t1 * t1)) +
                                ((q[2] * q[5]) * wl) / (t2 * t2);
            dndl = -down / sqrt(n2);
          }
        }
      }
    }
    dead = was_dead || invalid || unknown || unfit;
    // the wavefront form: the segment as prt_frame_optical_path has it, and at a selected row E, s, the OPD and the pupil
    // point as k_frame_wavefront_pupil has them, against the group's fixed sphere
    double seg = 0.0, nidx = 1.0, s_ext = 0.0, ep_d = 1.0, pupil_r = 1.0;
    SensVec ep = {0.0, 0.0, 0.0};
    bool hit = false;
    if constexpr (kOpd) {
      seg = sqrt(sv_dot(run, run));
      nidx = rows[PRT_COL_INDEX * ld + j];
      if (slot >= 0) {
        int lo = 0, hi = wave->n_groups;  // the last group q with first[q] <= slot
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (wave->first[mid] <= slot) lo = mid; else hi = mid;
        }
        const double* __restrict__ g = wave->groups + (int64_t)lo * SENS_OPD_GROUP;
        double e[3], opd = nan, p1 = nan, p2 = nan;
        pupil_r = g[5];
        if (!dead && wf_extend(rows, ld, j, g, g[3], s_ext, e)) {
          opd = (wave->opl[j] - nidx * s_ext) - g[4];
          ep = {e[0] - g[0], e[1] - g[1], e[2] - g[2]};
          p1 = ((ep.x * wave->e1[0] + ep.y * wave->e1[1]) + ep.z * wave->e1[2]) / pupil_r;
          p2 = ((ep.x * wave->e2[0] + ep.y * wave->e2[1]) + ep.z * wave->e2[2]) / pupil_r;
          ep_d = sv_dot(ep, d);
          hit = is_finite(opd) && is_finite(p1) && is_finite(p2);
        }
        wave->opd[slot] = hit ? opd : nan;
        wave->pupil[2 * slot] = hit ? p1 : nan;
        wave->pupil[2 * slot + 1] = hit ? p2 : nan;
      }
    }
    if (!dead) {
#pragma unroll 1
      for (int k = 0; k < K; ++k) {
        const SensTwist& tw = args.twist[k];
        SensVec dx = {0.0, 0.0, 0.0}, dd = {0.0, 0.0, 0.0}, start = {0.0, 0.0, 0.0};
        bool lin = false, idx = false;
        double dnu = 0.0;
        if constexpr (kDesign) {
          lin = (design->linear >> k) & 1u;
          idx = (design->index >> k) & 1u;
        }
        bool seeded = false, coloured = false;
        if constexpr (kLaunch) {
          const bool named = rid >= launch->lo[k] && rid < launch->hi[k];
          seeded = named && ((launch->seeds >> k) & 1u);
          coloured = named && ((launch->colour >> k) & 1u);
        }
        if (generation > 0) {
          double* __restrict__ s = state + (int64_t)k * kPlanes * n_ids + i;
          dx = {s[0], s[n_ids], s[2 * n_ids]};
          dd = {s[3 * n_ids], s[4 * n_ids], s[5 * n_ids]};
          if constexpr (kDesign) {
            if (idx) dnu = s[6 * n_ids];
          }
          // dn = w x n (a moved surface) + W (dx - u)
          const bool moved = (moved_there >> k) & 1u;
          SensVec dn = {0.0, 0.0, 0.0};
          if (there.h) {
            SensVec up = sens_velocity(tw, moved, xp);
            if constexpr (kDesign) {
              if (moved && lin) up = sv_add(up, sens_linear(design->S[k], tw, xp));
            }
            const SensVec y = sv_sub(dx, up);
            const double z0 = (there.h & 1) ? (a0[0] * y.x + a0[1] * y.y) + a0[2] * y.z : 0.0;
            const double z1 = (there.h & 2) ? (a1[0] * y.x + a1[1] * y.y) + a1[2] * y.z : 0.0;
            const double z2 = (there.h & 4) ? (a2[0] * y.x + a2[1] * y.y) + a2[2] * y.z : 0.0;
            const SensVec m = {((a0[0] * z0 + a1[0] * z1) + a2[0] * z2) / there.denom,
                               ((a0[1] * z0 + a1[1] * z1) + a2[1] * z2) / there.denom,
                               ((a0[2] * z0 + a1[2] * z1) + a2[2] * z2) / there.denom};
            const double along = sv_dot(there.n, m);
            dn = sv_scale(there.sign, sv_sub(m, sv_scale(along, there.n)));
          }
          if (moved) dn = sv_add(sv_cross({tw.w[0], tw.w[1], tw.w[2]}, there.n), dn);
          if constexpr (kDesign) {
            if (moved && lin) {  // - (I - n n^T) S^T n: the normal of a material point of the deformed surface
              const double* __restrict__ S = design->S[k];
              const SensVec& n = there.n;
              const SensVec q = {(S[0] * n.x + S[3] * n.y) + S[6] * n.z, (S[1] * n.x + S[4] * n.y) + S[7] * n.z,
                                 (S[2] * n.x + S[5] * n.y) + S[8] * n.z};
              dn = sv_sub(dn, sv_sub(q, sv_scale(sv_dot(n, q), n)));
            }
          }
          if (kind == SENS_REFRACT) {
            const double dci = -(sv_dot(dn, dp) + sv_dot(there.n, dd));
            const double dct = ((mu * mu) * ci) * dci / ct;
            const double dgamma = mu * dci - dct;
            dd = sv_add(sv_add(sv_scale(mu, dd), sv_scale(dgamma, there.n)), sv_scale(gamma, dn));
            if constexpr (kDesign) {
              if (idx) {  // the terms of dmu, after those of the geometry: dct and dgamma are linear in (dci, dmu)
                double dnt = (entering && ((index_there >> k) & 1u)) ? design->rate[k] : 0.0;
                if constexpr (kLaunch) {
                  if (coloured) dnt = entering ? launch->rate[k] * dndl : 0.0;
                }
                const double dmu = (dnu - mu * dnt) / nt_there;
                const double dct_mu = (mu * (1.0 - ci * ci)) * dmu / ct;  // dct = (mu^2 ci dci) / ct - dct_mu
                const double dgamma_mu = ci * dmu + dct_mu;
                dd = sv_add(dd, sv_add(sv_scale(dmu, dp), sv_scale(dgamma_mu, there.n)));
                dnu = dnt;
              }
            }
          } else if (kind == SENS_REFLECT) {
            const double turn = sv_dot(dd, there.n) + sv_dot(dp, dn);
            const SensVec back = sv_add(sv_scale(turn, there.n), sv_scale(there.nd, dn));
            dd = sv_sub(dd, sv_scale(2.0, back));
          }
          start = sv_add(dx, sv_scale(PRT_SENS_OFFSET, dd));
        }
        if constexpr (kLaunch) {  // the seed: the launch point moves with v + w x (o - c), the direction with w x d
          if (generation == 0 && seeded) {
            start = sens_velocity(tw, true, o);
            dd = sv_cross({tw.w[0], tw.w[1], tw.w[2]}, d);
          }
        }
        // the landing: dt = n.(u - do - t dd) / (n.d), dx = do + t dd + d dt
        SensVec u = sens_velocity(tw, (moved_here >> k) & 1u, x);
        if constexpr (kDesign) {
          if (((moved_here >> k) & 1u) && lin) u = sv_add(u, sens_linear(design->S[k], tw, x));
        }
        const SensVec reach = sv_add(start, sv_scale(t, dd));
        const double dt = sv_dot(here.n, sv_sub(u, reach)) / here.nd;
        dx = sv_add(reach, sv_scale(dt, d));
        double* __restrict__ s = state + (int64_t)k * kPlanes * n_ids + i;
        s[0] = dx.x; s[n_ids] = dx.y; s[2 * n_ids] = dx.z;
        s[3 * n_ids] = dd.x; s[4 * n_ids] = dd.y; s[5 * n_ids] = dd.z;
        if constexpr (kDesign) {
          if (idx) s[6 * n_ids] = dnu;  // (read by index parameters alone)
        }
        if (slot >= 0) {
          double* __restrict__ out = jacobian + (int64_t)k * 3 * n_selected + slot;
          out[0] = dx.x; out[n_selected] = dx.y; out[2 * n_selected] = dx.z;
          if constexpr (kLaunch) {
            double* __restrict__ slope = slopes + (int64_t)k * 3 * n_selected + slot;
            slope[0] = dd.x; slope[n_selected] = dd.y; slope[2 * n_selected] = dd.z;
          }
        }
        if constexpr (kOpd) {  // dL = dL_prev + dnu len + n d.(dx - start); then the wavefront change at the fixed sphere
          const double before = generation > 0 ? s[7 * n_ids] : 0.0;
          const double dL = (before + dnu * seg) + nidx * sv_dot(d, sv_sub(dx, start));
          s[7 * n_ids] = dL;
          if (slot >= 0) {
            double dfield = nan, dopd = nan, dp1 = nan, dp2 = nan;
            if (hit) {
              dfield = (dL - s_ext * dnu) - nidx * sv_dot(d, dx);
              const SensVec y = sv_sub(dx, sv_scale(s_ext, dd));
              const double ds = sv_dot(ep, y) / ep_d;
              const SensVec dE = sv_sub(y, sv_scale(ds, d));
              dp1 = ((dE.x * wave->e1[0] + dE.y * wave->e1[1]) + dE.z * wave->e1[2]) / pupil_r;
              dp2 = ((dE.x * wave->e2[0] + dE.y * wave->e2[1]) + dE.z * wave->e2[2]) / pupil_r;
              dopd = dfield + nidx * sv_dot(d, dE);
            }
            wave->dfield[(int64_t)k * n_selected + slot] = dfield;
            wave->dopd[(int64_t)k * n_selected + slot] = dopd;
            wave->dpupil[(int64_t)(2 * k) * n_selected + slot] = dp1;
            wave->dpupil[(int64_t)(2 * k + 1) * n_selected + slot] = dp2;
          }
        }
      }
    }
    // a ray is counted once: it is NaN from there on
    unknown = unknown && !was_dead;
    invalid = invalid && !was_dead && !unknown;
    unfit = unfit && !was_dead;
  }
  if (dead && slot >= 0)
    for (int k = 0; k < K; ++k) {
      double* __restrict__ out = jacobian + (int64_t)k * 3 * n_selected + slot;
      out[0] = nan; out[n_selected] = nan; out[2 * n_selected] = nan;
      if constexpr (kLaunch) {
        double* __restrict__ slope = slopes + (int64_t)k * 3 * n_selected + slot;
        slope[0] = nan; slope[n_selected] = nan; slope[2 * n_selected] = nan;
      }
      if constexpr (kOpd) {
        wave->dfield[(int64_t)k * n_selected + slot] = nan;
        wave->dopd[(int64_t)k * n_selected + slot] = nan;
        wave->dpupil[(int64_t)(2 * k) * n_selected + slot] = nan;
        wave->dpupil[(int64_t)(2 * k + 1) * n_selected + slot] = nan;
      }
    }
  if constexpr (kOpd) {
    if (dead && !joined && slot >= 0) {  // (a row the join refused never reached the block above)
      wave->opd[slot] = nan; wave->pupil[2 * slot] = nan; wave->pupil[2 * slot + 1] = nan;
    }
  }
  if (i >= 0) last_row[i] = dead ? -1 - j : j;  // (also for a row the status word refuses: the next launch reads this one's)
  flag[0] = unknown; flag[1] = invalid; flag[2] = unfit; flag[3] = reflection;
}

__global__ void __launch_bounds__(kSensBlock)
k_sens_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count, int generation,
            double id0, int64_t n_ids, SensArgs args, const SensSurface* __restrict__ table, double* __restrict__ state,
            int64_t* __restrict__ last_row, int* __restrict__ stamp, SensWords* __restrict__ words,
            const int64_t* __restrict__ row_slot, int64_t n_selected, double* __restrict__ jacobian) {
  const int64_t j = start + (int64_t)blockIdx.x * kSensBlock + threadIdx.x;
  bool flag[SENS_COUNTERS] = {};
  if (j < start + count)
    sens_row<false>(rows, ld, n_rows, j, generation, id0, n_ids, args, table, state, last_row, stamp, &words->status,
                    row_slot, n_selected, jacobian, flag, nullptr);
  fresnel_count(flag, words->count);
}

__global__ void __launch_bounds__(kSensBlock)
k_sens_design_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count,
                   int generation, double id0, int64_t n_ids, SensArgs args, SensDesign design,
                   const SensSurface* __restrict__ table, double* __restrict__ state, int64_t* __restrict__ last_row,
                   int* __restrict__ stamp, SensWords* __restrict__ words, const int64_t* __restrict__ row_slot,
                   int64_t n_selected, double* __restrict__ jacobian) {
  const int64_t j = start + (int64_t)blockIdx.x * kSensBlock + threadIdx.x;
  bool flag[SENS_COUNTERS] = {};
  if (j < start + count)
    sens_row<true>(rows, ld, n_rows, j, generation, id0, n_ids, args, table, state, last_row, stamp, &words->status,
                   row_slot, n_selected, jacobian, flag, &design);
  fresnel_count(flag, words->count);
}

__global__ void __launch_bounds__(kSensBlock)
k_sens_opd_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count, int generation,
                double id0, int64_t n_ids, SensArgs args, SensDesign design, SensOpd wave,
                const SensSurface* __restrict__ table, double* __restrict__ state, int64_t* __restrict__ last_row,
                int* __restrict__ stamp, SensWords* __restrict__ words, const int64_t* __restrict__ row_slot,
                int64_t n_selected, double* __restrict__ jacobian) {
  const int64_t j = start + (int64_t)blockIdx.x * kSensBlock + threadIdx.x;
  bool flag[SENS_COUNTERS] = {};
  if (j < start + count)
    sens_row<true, true>(rows, ld, n_rows, j, generation, id0, n_ids, args, table, state, last_row, stamp, &words->status,
                         row_slot, n_selected, jacobian, flag, &design, &wave);
  fresnel_count(flag, words->count);
}

__global__ void __launch_bounds__(kSensBlock)
k_sens_launch_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count,
                   int generation, double id0, int64_t n_ids, SensArgs args, SensDesign design, SensLaunch launch,
                   const SensSurface* __restrict__ table, const SensGlass* __restrict__ glass, double* __restrict__ state,
                   int64_t* __restrict__ last_row, int* __restrict__ stamp, SensWords* __restrict__ words,
                   const int64_t* __restrict__ row_slot, int64_t n_selected, double* __restrict__ jacobian,
                   double* __restrict__ slopes) {
  const int64_t j = start + (int64_t)blockIdx.x * kSensBlock + threadIdx.x;
  bool flag[SENS_COUNTERS] = {};
  if (j < start + count)
    sens_row<true, false, true>(rows, ld, n_rows, j, generation, id0, n_ids, args, table, state, last_row, stamp,
                                &words->status, row_slot, n_selected, jacobian, flag, &design, nullptr, &launch, glass,
                                slopes);
  fresnel_count(flag, words->count);
}

__global__ void __launch_bounds__(kSensBlock)
k_sens_launch_opd_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count,
                       int generation, double id0, int64_t n_ids, SensArgs args, SensDesign design, SensOpd wave,
                       SensLaunch launch, const SensSurface* __restrict__ table, const SensGlass* __restrict__ glass,
                       double* __restrict__ state, int64_t* __restrict__ last_row, int* __restrict__ stamp,
                       SensWords* __restrict__ words, const int64_t* __restrict__ row_slot, int64_t n_selected,
                       double* __restrict__ jacobian, double* __restrict__ slopes) {
  const int64_t j = start + (int64_t)blockIdx.x * kSensBlock + threadIdx.x;
  bool flag[SENS_COUNTERS] = {};
  if (j < start + count)
    sens_row<true, true, true>(rows, ld, n_rows, j, generation, id0, n_ids, args, table, state, last_row, stamp,
                               &words->status, row_slot, n_selected, jacobian, flag, &design, &wave, &launch, glass,
                               slopes);
  fresnel_count(flag, words->count);
}

// ---- the group sums ------------------------------------------------------------------------------------------------------
// entries of a group, K parameters: count, sum w, sum w x (3), sum w |x - pivot|^2, sum w dx_k (3 K, k-major), sum w (x - pivot).dx_k (K),
// sum w dx_j.dx_k for k <= j (K (K + 1) / 2, row-major lower triangle)
static int sens_entries(int K) { return SENS_FIXED + 3 * K + K + K * (K + 1) / 2; }

// what slot s (row r, finite throughout) adds to entry e
__device__ __forceinline__ double sens_entry(int e, int K, double w, const SensVec& x, const SensVec& pivot,
                                             const double* __restrict__ jacobian, int64_t n_selected, int64_t s) {
  if (e == 0) return 1.0;
  if (e == 1) return w;
  if (e < 5) return w * (e == 2 ? x.x : e == 3 ? x.y : x.z);
  if (e == 5) { const SensVec r = sv_sub(x, pivot); return w * sv_dot(r, r); }
  e -= SENS_FIXED;
  if (e < 3 * K) return w * jacobian[(int64_t)e * n_selected + s];
  e -= 3 * K;
  const auto column = [&](int k) -> SensVec {
    const double* __restrict__ c = jacobian + (int64_t)k * 3 * n_selected + s;
    return {c[0], c[n_selected], c[2 * n_selected]};
  };
  if (e < K) return w * sv_dot(sv_sub(x, pivot), column(e));
  e -= K;
  int row = 0;
  while ((row + 1) * (row + 2) / 2 <= e) ++row;
  return w * sv_dot(column(row), column(e - row * (row + 1) / 2));
}

// workgroup (chunk, group): slots [first[group] + 256 chunk, ...) of the group; its partial sums to
// partials[(group * chunks + chunk) * entries + e], waves added in order
__global__ void __launch_bounds__(kSensBlock)
k_sens_partials(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ selected,
                int64_t n_selected, const int64_t* __restrict__ first, int K, int weight_column,
                const double* __restrict__ pivots, const double* __restrict__ jacobian, double* __restrict__ partials,
                int* status) {
  __shared__ double red[SENS_MAX_ENTRIES][kSensWaves];
  const int group = blockIdx.y, entries = SENS_FIXED + 3 * K + K + K * (K + 1) / 2;
  const int64_t s = first[group] + (int64_t)blockIdx.x * kSensBlock + threadIdx.x;
  double* __restrict__ out = partials + ((int64_t)group * gridDim.x + blockIdx.x) * entries;
  bool live = s < first[group + 1] && s < n_selected;
  double w = 0.0;
  SensVec x = {0.0, 0.0, 0.0};
  const SensVec pivot = {pivots[3 * group], pivots[3 * group + 1], pivots[3 * group + 2]};
  if (live) {
    const int64_t r = selected[s];
    if (r < 0 || r >= n_rows) {
      atomicOr(status, SENS_BAD_SELECTION);
      live = false;
    } else {
      w = weight_column < 0 ? 1.0 : rows[weight_column * ld + r];
      x = sv_col(rows, ld, PRT_COL_X1, r);
      live = is_finite(w) && sv_finite(x);
      for (int c = 0; c < 3 * K; ++c) live = live && is_finite(jacobian[(int64_t)c * n_selected + s]);
    }
  }
  for (int e = 0; e < entries; ++e) {
    double v = live ? sens_entry(e, K, w, x, pivot, jacobian, n_selected, s) : 0.0;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[e][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < entries; e += kSensBlock) {
    double sum = red[e][0];
    for (int wave = 1; wave < kSensWaves; ++wave) sum += red[e][wave];
    out[e] = sum;
  }
}

// one wave per (group, entry): lane l adds the group's partials l, l + 64, ... in that order, then the butterfly: a fixed
// order, and no lane walks thousands of workgroups alone
__global__ void __launch_bounds__(64)
k_sens_fold(const double* __restrict__ partials, int chunks, int entries, int n_groups, double* __restrict__ sums) {
  const int64_t at = blockIdx.x;
  if (at >= (int64_t)n_groups * entries) return;
  const int64_t group = at / entries, e = at % entries;
  double sum = 0.0;
  for (int chunk = threadIdx.x; chunk < chunks; chunk += 64) sum += partials[(group * chunks + chunk) * entries + e];
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if (threadIdx.x == 0) sums[at] = sum;
}

// ---- the wavefront sums ----------------------------------------------------------------------------------------------------
// entries of a group, K parameters and J Zernike terms, over the selected rows that are finite throughout and met the sphere:
// count, rows that missed the sphere, sum w, sum w OPD, sum w OPD^2 (OPD about the pivot); Z^T W y, column-major, for the
// K + 3 columns y = dfield_k and n u_c (J (K + 3)); sum w dopd_k, sum w OPD dopd_k, sum w dfield_k, sum w OPD dfield_k (K each);
// sum w dfield_j dfield_k for k <= j (row-major lower triangle).
// Every entry is a sum over rows of L[l] * R[r], two columns of a tile that a workgroup keeps in LDS for 64 rows at a time:
//   L: Z_1..Z_J, 1, OPD, dfield_k (J + 2 + K)      R: w dfield_k, w n u_c, w dopd_k, w, w OPD, live, missed (2 K + 7)
// A thread owns up to four entries and walks the tile's rows in order, four independent chains; the basis is evaluated
// once a row, by the wave whose rows are staged.  (k_frame_zernike owns one entry a thread over thousands of rows in few
// workgroups; here a workgroup has 256 rows and the grid has one workgroup per 256 rows, so the chains are short and many.)
enum { SENS_OPD_FIXED = 5, SENS_OPD_TILE = 64 };
static int sens_opd_entries(int K, int J) { return SENS_OPD_FIXED + J * (K + 3) + 4 * K + K * (K + 1) / 2; }
enum { SENS_OPD_MAX_ENTRIES = SENS_OPD_FIXED + WF_MAX_TERMS * (SENS_MAX_PARAMETERS + 3) + 4 * SENS_MAX_PARAMETERS +
                              SENS_MAX_PARAMETERS * (SENS_MAX_PARAMETERS + 1) / 2 };
static const int kOpdEntriesPerThread = (SENS_OPD_MAX_ENTRIES + kSensBlock - 1) / kSensBlock;
__host__ __device__ constexpr int sens_opd_stride(int K, int J) { return (J + 3 * K + 9) | 1; }

// the columns (l of L, r of R) of entry e
__device__ __forceinline__ void sens_opd_entry(int e, int K, int J, int& l, int& r) {
  const int one = J, opd = J + 1, w = 2 * K + 3, w_opd = 2 * K + 4;
  if (e < SENS_OPD_FIXED) {
    l = e == 4 ? opd : one;
    r = e == 0 ? 2 * K + 5 : e == 1 ? 2 * K + 6 : e == 2 ? w : w_opd;
    return;
  }
  e -= SENS_OPD_FIXED;
  if (e < J * (K + 3)) { l = e % J; r = e / J; return; }
  e -= J * (K + 3);
  if (e < 4 * K) {
    const int which = e / K, k = e % K;  // dopd, OPD dopd, dfield, OPD dfield
    l = (which & 1) ? opd : one;
    r = which < 2 ? K + 3 + k : k;
    return;
  }
  e -= 4 * K;
  int row = 0;
  while ((row + 1) * (row + 2) / 2 <= e) ++row;
  l = J + 2 + row;
  r = e - row * (row + 1) / 2;
}

// workgroup (chunk, group): slots [first[group] + 256 chunk, ...) of the group; its partial sums to
// partials[(group * chunks + chunk) * entries + e]
__global__ void __launch_bounds__(kSensBlock)
k_sens_opd_partials(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ selected,
                    int64_t n_selected, const int64_t* __restrict__ first, int K, int J, int weight_column,
                    const double* __restrict__ jacobian, const double* __restrict__ opd, const double* __restrict__ pupil,
                    const double* __restrict__ dfield, const double* __restrict__ dopd, double* __restrict__ partials,
                    int* status) {
  extern __shared__ double opd_tile[];  // [SENS_OPD_TILE][stride]: L then R of each row
  const int group = blockIdx.y, entries = SENS_OPD_FIXED + J * (K + 3) + 4 * K + K * (K + 1) / 2;
  const int stride = sens_opd_stride(K, J), n_left = J + 2 + K;
  const int64_t begin = first[group] + (int64_t)blockIdx.x * kSensBlock;
  const int64_t end = first[group + 1] < n_selected ? first[group + 1] : n_selected;
  double* __restrict__ out = partials + ((int64_t)group * gridDim.x + blockIdx.x) * entries;
  int el[kOpdEntriesPerThread], er[kOpdEntriesPerThread];
  double acc[kOpdEntriesPerThread];
#pragma unroll
  for (int q = 0; q < kOpdEntriesPerThread; ++q) {
    const int e = threadIdx.x + q * kSensBlock;
    el[q] = er[q] = -1;
    if (e < entries) sens_opd_entry(e, K, J, el[q], er[q]);
    acc[q] = 0.0;
  }
  for (int sub = 0; sub < kSensWaves; ++sub) {
    const int64_t base = begin + (int64_t)sub * SENS_OPD_TILE;
    if (base >= end) break;  // (the same for every thread of the workgroup)
    const int here = (int)(end - base < SENS_OPD_TILE ? end - base : SENS_OPD_TILE);
    if ((int)(threadIdx.x >> 6) == sub) {
      const int lane = threadIdx.x & 63;
      double* __restrict__ L = opd_tile + lane * stride;
      double* __restrict__ R = L + n_left;
      const int64_t s = base + lane;
      bool live = false, missed = false;
      double w = 0.0, v = 0.0, nu[3] = {0.0, 0.0, 0.0};
      double z[WF_MAX_TERMS];
#pragma unroll
      for (int k = 0; k < WF_MAX_TERMS; ++k) z[k] = 0.0;
      if (lane < here) {
        const int64_t r = selected[s];
        if (r < 0 || r >= n_rows) {
          atomicOr(status, SENS_BAD_SELECTION);
        } else {
          w = weight_column < 0 ? 1.0 : rows[weight_column * ld + r];
          bool followed = is_finite(w) && sv_finite(sv_col(rows, ld, PRT_COL_X1, r));
          for (int c = 0; c < 3 * K; ++c) followed = followed && is_finite(jacobian[(int64_t)c * n_selected + s]);
          v = opd[s];
          const double px = pupil[2 * s], py = pupil[2 * s + 1];
          live = followed && is_finite(v) && is_finite(px) && is_finite(py);
          missed = followed && !live;
          for (int k = 0; k < K; ++k)
            live = live && is_finite(dfield[(int64_t)k * n_selected + s]) && is_finite(dopd[(int64_t)k * n_selected + s]);
          if (live) {
            wf_zernike(px, py, z);
            const double n = rows[PRT_COL_INDEX * ld + r];
            const SensVec u = sv_col(rows, ld, PRT_COL_XTILT, r);
            nu[0] = n * u.x; nu[1] = n * u.y; nu[2] = n * u.z;
            live = is_finite(nu[0]) && is_finite(nu[1]) && is_finite(nu[2]);
          }
        }
      }
      if (!live) { w = 0.0; v = 0.0; }
#pragma unroll
      for (int k = 0; k < WF_MAX_TERMS; ++k)
        if (k < J) L[k] = live ? z[k] : 0.0;
      L[J] = 1.0;
      L[J + 1] = v;
      for (int k = 0; k < K; ++k) {
        const double f = live ? dfield[(int64_t)k * n_selected + s] : 0.0;
        const double o = live ? dopd[(int64_t)k * n_selected + s] : 0.0;
        L[J + 2 + k] = f;
        R[k] = w * f;
        R[K + 3 + k] = w * o;
      }
      for (int c = 0; c < 3; ++c) R[K + c] = live ? w * nu[c] : 0.0;
      R[2 * K + 3] = w;
      R[2 * K + 4] = w * v;
      R[2 * K + 5] = live ? 1.0 : 0.0;
      R[2 * K + 6] = missed ? 1.0 : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kOpdEntriesPerThread; ++q) {
      if (el[q] < 0) continue;
      const double* __restrict__ a = opd_tile + el[q];
      const double* __restrict__ b = opd_tile + n_left + er[q];
      double c = acc[q];
      for (int k = 0; k < here; ++k) c += a[k * stride] * b[k * stride];
      acc[q] = c;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kOpdEntriesPerThread; ++q)
    if (el[q] >= 0) out[threadIdx.x + q * kSensBlock] = acc[q];
}

// ---- entry points: what the four forms share ---------------------------------------------------------------------------------
// what every entry point is given
struct SensCall {
  int device; const double* rows; int64_t ld; const int64_t* rows_per_generation; int n_generations; double id0; int64_t n_ids;
  const prt_prim* surfaces; int n_surfaces; const double* twists; const int64_t* parameter_ids; const int32_t* parameter_first;
  int n_parameters; const int64_t* row_slot; const int64_t* selected; int64_t n_selected; const int64_t* group_first;
  int n_groups, weight_column; const double* pivots; double *jacobian_out, *sums_out; int64_t* record_out;
  void *workspace, *stream;
};
// the design form's arguments on the host: linear HOST (K, 9), index_rates HOST K, index_ids and index_first as parameter_*
struct SensDesignCall { const double* linear; const double* index_rates; const int64_t* index_ids; const int32_t* index_first; };
// the wavefront form's arguments on the host: opl DEVICE n_rows; groups HOST (n_groups, 6); axes HOST 9; the outputs DEVICE
struct SensOpdCall {
  const double* opl; const double* groups; const double* axes; int n_terms;
  double *dfield, *dopd, *dpupil, *opd, *pupil, *sums;
};
// the launch form's arguments on the host: ranges HOST (K, 2), flags HOST K (bit 0 seeds the launch, bit 1 changes the
// wavelength), rates HOST K, materials HOST n_materials (what prt_prim.material indexes); slopes DEVICE (K, 3, n_selected)
struct SensLaunchCall {
  const double* ranges; const int32_t* flags; const double* rates; const prt_material* materials; int n_materials;
  double* slopes;
};

// ---- the workspace: one layout for every form -----------------------------------------------------------------------------------
struct SensSizes { int64_t n_ids; int n_surfaces, n_parameters, n_groups; int64_t max_group_rows; };
// every form: the words, the surface table, group_first, the pivots, the state, per id its previous row, the partials of
// the sums, the stamps.  The wavefront form has behind that the group records and the partials of its own sums; the
// launch form, behind everything the other forms carve, the glass table.  `end`: the first byte the call leaves alone
struct SensWork {
  SensWords* words; SensSurface* table; int64_t* first; double* pivots; double* state; int64_t* last_row; int* stamp; double* partials;
  double *opd_groups, *opd_partials;
  SensGlass* glass;
  char* end;
};

static int64_t sens_chunks(int64_t max_group_rows) { return (max_group_rows + kSensBlock - 1) / kSensBlock; }

static bool sens_sizes_ok(const SensSizes& s) {
  return join_n_ids_ok(s.n_ids) && s.n_surfaces >= 1 && s.n_surfaces <= (1 << 20) && s.n_parameters >= 1 &&
         s.n_parameters <= SENS_MAX_PARAMETERS && s.n_groups >= 1 && s.n_groups <= 65535 && s.max_group_rows >= 0 &&
         sens_chunks(s.max_group_rows) <= 0x7fffffff;
}

// `planes` of state a parameter and id (6 rigid, 7 design, 8 with dL); n_terms: the wavefront's Zernike terms, or 0
static SensWork sens_layout(void* workspace, const SensSizes& s, int planes, int n_terms, bool with_glasses) {
  const int64_t group_chunks = (int64_t)s.n_groups * sens_chunks(s.max_group_rows);
  const auto to8 = [](char* at) { return ((uintptr_t)at + 7) & ~(uintptr_t)7; };
  SensWork w;
  w.words = (SensWords*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  w.table = (SensSurface*)((char*)w.words + 64);
  w.first = (int64_t*)(w.table + s.n_surfaces);
  w.pivots = (double*)(w.first + s.n_groups + 1);
  w.state = w.pivots + 3 * (int64_t)s.n_groups;
  w.last_row = (int64_t*)(w.state + planes * (int64_t)s.n_parameters * s.n_ids);
  w.partials = (double*)(w.last_row + s.n_ids);
  w.stamp = (int*)(w.partials + group_chunks * sens_entries(s.n_parameters));
  w.end = (char*)(w.stamp + s.n_ids);
  w.opd_groups = w.opd_partials = nullptr;
  if (n_terms) {
    w.opd_groups = (double*)to8(w.end);
    w.opd_partials = w.opd_groups + (int64_t)s.n_groups * SENS_OPD_GROUP;
    w.end = (char*)(w.opd_partials + group_chunks * sens_opd_entries(s.n_parameters, n_terms));
  }
  w.glass = nullptr;
  if (with_glasses) {
    w.glass = (SensGlass*)to8(w.end);
    w.end = (char*)(w.glass + s.n_surfaces);
  }
  return w;
}

// the layout from address 0, and 64 bytes for the alignment of the words
static int64_t sens_workspace_bytes(const SensSizes& s, int planes, int n_terms, bool with_glasses) {
  if (!sens_sizes_ok(s)) return PRT_ERR_ARG;
  return (int64_t)(uintptr_t)sens_layout(nullptr, s, planes, n_terms, with_glasses).end + 64;
}

extern "C" int64_t prt_frame_sensitivity_workspace_bytes(int64_t n_ids, int n_surfaces, int n_parameters, int n_groups,
                                                         int64_t max_group_rows) {
  return sens_workspace_bytes({n_ids, n_surfaces, n_parameters, n_groups, max_group_rows}, 6, 0, false);
}

extern "C" int64_t prt_frame_design_sensitivity_workspace_bytes(int64_t n_ids, int n_surfaces, int n_parameters,
                                                                int n_groups, int64_t max_group_rows) {
  return sens_workspace_bytes({n_ids, n_surfaces, n_parameters, n_groups, max_group_rows}, 7, 0, false);
}

extern "C" int64_t prt_frame_opd_sensitivity_workspace_bytes(int64_t n_ids, int n_surfaces, int n_parameters, int n_groups,
                                                             int64_t max_group_rows, int n_terms) {
  if (n_terms < 1 || n_terms > WF_MAX_TERMS) return PRT_ERR_ARG;
  return sens_workspace_bytes({n_ids, n_surfaces, n_parameters, n_groups, max_group_rows}, 8, n_terms, false);
}

extern "C" int64_t prt_frame_launch_sensitivity_workspace_bytes(int64_t n_ids, int n_surfaces, int n_parameters,
                                                                int n_groups, int64_t max_group_rows, int n_terms) {
  if (n_terms < 0 || n_terms > WF_MAX_TERMS) return PRT_ERR_ARG;
  return sens_workspace_bytes({n_ids, n_surfaces, n_parameters, n_groups, max_group_rows}, n_terms ? 8 : 7, n_terms, true);
}

// ---- the steps of a call, in the order sens_run takes them ------------------------------------------------------------------------
// the buffers and the sizes; the number of rows (or an error) and the rows of the largest group
static int64_t sens_check(const SensCall& c, const SensDesignCall* design, const SensOpdCall* wave, int64_t& max_group_rows) {
  const int64_t n_rows = join_rows(c.rows_per_generation, c.n_generations, c.ld, kSensBlock, "sensitivity");
  if (n_rows < 0) return n_rows;
  if (!c.record_out || !c.workspace || !c.sums_out || !c.surfaces || !c.twists || !c.parameter_first || !c.group_first ||
      !c.pivots || c.n_selected < 0 || c.n_selected > n_rows || (n_rows && (!c.rows || !c.row_slot)) ||
      (c.n_selected && (!c.selected || !c.jacobian_out)) ||
      (design && (!design->linear || !design->index_rates || !design->index_first)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (wave) {
    if (!wave->groups || !wave->axes || !wave->sums || (n_rows && !wave->opl) ||
        (c.n_selected && (!wave->dfield || !wave->dopd || !wave->dpupil || !wave->opd || !wave->pupil)))
      return fail(PRT_ERR_ARG, "bad buffers");
    if (wave->n_terms < 1 || wave->n_terms > WF_MAX_TERMS) return fail(PRT_ERR_ARG, "opd sensitivity: 1 to 36 Zernike terms");
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(wave->axes[k])) return fail(PRT_ERR_ARG, "opd sensitivity: axes finite");
  }
  const int rc = join_ids(c.id0, c.n_ids);
  if (rc) return rc;
  if (c.n_parameters < 1 || c.n_parameters > SENS_MAX_PARAMETERS)
    return fail(PRT_ERR_ARG, "sensitivity: 1 to 16 parameters a call");
  if (c.n_groups < 1 || c.n_groups > 65535) return fail(PRT_ERR_ARG, "sensitivity: 1 to 65535 groups");
  if (c.weight_column < -1 || c.weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "sensitivity: weight_column");
  if (c.n_surfaces < 1 || c.n_surfaces > (1 << 20)) return fail(PRT_ERR_ARG, "sensitivity: 1 to 2^20 surfaces in the table");
  max_group_rows = 0;
  if (c.group_first[0] != 0 || c.group_first[c.n_groups] != c.n_selected)
    return fail(PRT_ERR_ARG, "sensitivity: group_first runs from 0 to n_selected");
  for (int g = 0; g < c.n_groups; ++g) {
    if (c.group_first[g + 1] < c.group_first[g]) return fail(PRT_ERR_ARG, "sensitivity: group_first ascends");
    max_group_rows = std::max(max_group_rows, c.group_first[g + 1] - c.group_first[g]);
  }
  for (int k = 0; k < 3 * c.n_groups; ++k)
    if (!(std::fabs(c.pivots[k]) < PRT_INF)) return fail(PRT_ERR_ARG, "sensitivity: pivots finite");
  if (wave)  // (a group without rows has a NaN record and no row reads it; a pupil radius must divide)
    for (int g = 0; g < c.n_groups; ++g) {
      const double radius = wave->groups[SENS_OPD_GROUP * g + 5];
      if (c.group_first[g + 1] > c.group_first[g] && !(radius > 0.0 && radius < PRT_INF))
        return fail(PRT_ERR_ARG, "opd sensitivity: a group's pupil radius is not a positive number");
    }
  return n_rows;
}

// the surface table: of every primitive what world_normal_len reads, no bits yet
static int sens_table(const SensCall& c, std::vector<SensSurface>& table) {
  table.resize((size_t)c.n_surfaces);
  for (int s = 0; s < c.n_surfaces; ++s) {
    const prt_prim& pr = c.surfaces[s];
    if (pr.type < PRT_PRIM_SPHERE || pr.type > PRT_PRIM_PARABOLOID || (pr.normal_scale != 1 && pr.normal_scale != -1))
      return fail(PRT_ERR_ARG, "sensitivity: a surface of unknown kind or normal_scale");
    if (s && !(c.surfaces[s - 1].surface_id < pr.surface_id))
      return fail(PRT_ERR_ARG, "sensitivity: the surface table is sorted by id, ids distinct");
    SensSurface& out = table[s];
    std::memset(&out, 0, sizeof(out));
    for (int k = 0; k < 16; ++k) {
      if (!(std::fabs(pr.minv[k]) < PRT_INF)) return fail(PRT_ERR_ARG, "sensitivity: a surface's minv is not finite");
      out.minv[k] = pr.minv[k];
    }
    for (int k = 0; k < 6; ++k) out.params[k] = pr.params[k];
    out.surface_id = (double)pr.surface_id;
    out.type = pr.type;
    out.normal_scale = pr.normal_scale;
  }
  return PRT_OK;
}

// bit k of `by` (moved_by or index_by) in the table's entry of each of ids[from, to), found by bisection of the sorted
// surfaces; `refusal`: what is said of an id that no surface has
static int sens_mark(const SensCall& c, const int64_t* ids, int from, int to, uint32_t SensSurface::*by, int k,
                     std::vector<SensSurface>& table, const char* refusal) {
  for (int at = from; at < to; ++at) {
    int lo = 0, hi = c.n_surfaces;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (c.surfaces[mid].surface_id < ids[at]) lo = mid + 1; else hi = mid;
    }
    if (lo == c.n_surfaces || c.surfaces[lo].surface_id != ids[at]) return fail(PRT_ERR_ARG, refusal);
    table[lo].*by |= 1u << k;
  }
  return PRT_OK;
}

// the rigid parameters: the twists, and which surfaces each moves
static int sens_rigid(const SensCall& c, SensArgs& args, std::vector<SensSurface>& table) {
  std::memset(&args, 0, sizeof(args));
  args.n_parameters = c.n_parameters;
  args.n_surfaces = c.n_surfaces;
  if (c.parameter_first[0] != 0) return fail(PRT_ERR_ARG, "sensitivity: parameter_first starts at 0");
  for (int k = 0; k < c.n_parameters; ++k) {
    const int from = c.parameter_first[k], to = c.parameter_first[k + 1];
    if (to < from || to - from > SENS_MAX_IDS || (to > from && !c.parameter_ids))
      return fail(PRT_ERR_ARG, "sensitivity: at most 64 surface ids a parameter");
    for (int i = 0; i < 9; ++i) {
      const double value = c.twists[9 * k + i];
      if (!(std::fabs(value) < PRT_INF)) return fail(PRT_ERR_ARG, "sensitivity: a twist is not finite");
      (i < 3 ? args.twist[k].v[i] : i < 6 ? args.twist[k].w[i - 3] : args.twist[k].c[i - 6]) = value;
    }
    const int rc = sens_mark(c, c.parameter_ids, from, to, &SensSurface::moved_by, k, table,
                             "sensitivity: a parameter moves a surface that is not in the table");
    if (rc) return rc;
  }
  return PRT_OK;
}

// the design part: S and the index rate per parameter, and which surfaces' index each changes
static int sens_design(const SensCall& c, const SensDesignCall& d, SensDesign& shape, std::vector<SensSurface>& table) {
  if (d.index_first[0] != 0) return fail(PRT_ERR_ARG, "design sensitivity: index_first starts at 0");
  for (int k = 0; k < c.n_parameters; ++k) {
    for (int i = 0; i < 9; ++i) {
      const double value = d.linear[9 * k + i];
      if (!(std::fabs(value) < PRT_INF)) return fail(PRT_ERR_ARG, "design sensitivity: linear is not finite");
      shape.S[k][i] = value;
      if (value != 0.0) shape.linear |= 1u << k;
    }
    if (!(std::fabs(d.index_rates[k]) < PRT_INF)) return fail(PRT_ERR_ARG, "design sensitivity: an index rate is not finite");
    shape.rate[k] = d.index_rates[k];
    const int from = d.index_first[k], to = d.index_first[k + 1];
    if (to < from || to - from > SENS_MAX_IDS || (to > from && !d.index_ids))
      return fail(PRT_ERR_ARG, "design sensitivity: at most 64 surface ids an index parameter");
    const int rc = sens_mark(c, d.index_ids, from, to, &SensSurface::index_by, k, table,
                             "design sensitivity: an index parameter names a surface that is not in the table");
    if (rc) return rc;
    if (to > from) shape.index |= 1u << k;
  }
  return PRT_OK;
}

// the launch part: the rays each parameter names and what it does to them (the seeds), and the glass behind every surface
static int sens_launch(const SensCall& c, const SensLaunchCall& l, SensLaunch& seed, SensDesign& shape,
                       std::vector<SensGlass>& glasses) {
  if (!l.ranges || !l.flags || !l.rates || !l.materials || (c.n_selected && !l.slopes)) return fail(PRT_ERR_ARG, "bad buffers");
  for (int k = 0; k < c.n_parameters; ++k) {
    const double lo = l.ranges[2 * k], hi = l.ranges[2 * k + 1];
    if (l.flags[k] < 0 || l.flags[k] > 3) return fail(PRT_ERR_ARG, "launch sensitivity: flags are 0 to 3");
    if (!(lo <= hi)) return fail(PRT_ERR_ARG, "launch sensitivity: a parameter's ray ids [lo, hi) are not a range");
    if (!(std::fabs(l.rates[k]) < PRT_INF)) return fail(PRT_ERR_ARG, "launch sensitivity: a wavelength rate is not finite");
    if (l.flags[k] && c.parameter_first[k + 1] != c.parameter_first[k])
      return fail(PRT_ERR_ARG, "launch sensitivity: a launch parameter names no surfaces");
    seed.lo[k] = lo; seed.hi[k] = hi; seed.rate[k] = l.rates[k];
    if (l.flags[k] & 1) seed.seeds |= 1u << k;
    if (l.flags[k] & 2) { seed.colour |= 1u << k; shape.index |= 1u << k; }  // (the dnu plane is the parameter's)
  }
  glasses.resize((size_t)c.n_surfaces);
  for (int s = 0; s < c.n_surfaces; ++s) {
    const int m = c.surfaces[s].material;
    if (m < 0 || m >= l.n_materials) return fail(PRT_ERR_ARG, "launch sensitivity: a surface's material is not in materials");
    const prt_material& mat = l.materials[m];
    std::memset(&glasses[s], 0, sizeof(SensGlass));
    if (mat.kind == PRT_MAT_SELLMEIER) {
      for (int i = 0; i < 6; ++i) {
        if (!(std::fabs(mat.coef[i]) < PRT_INF)) return fail(PRT_ERR_ARG, "launch sensitivity: a Sellmeier coefficient is not finite");
        glasses[s].coef[i] = mat.coef[i];
      }
    } else if (seed.colour && (mat.kind < PRT_MAT_NONE || mat.kind > PRT_MAT_CONST_INDEX)) {
      return fail(PRT_ERR_ARG, "launch sensitivity: a wavelength parameter needs glasses whose dispersion the device has "
                               "(a table or host material is in the table)");
    }
    glasses[s].kind = mat.kind;
  }
  return PRT_OK;
}

// the uploads: what the kernels read from the workspace, and the words and stamps cleared
static int sens_upload(const SensCall& c, const SensWork& w, const std::vector<SensSurface>& table,
                       const std::vector<SensGlass>& glasses, const SensOpdCall* wave) {
  hipStream_t st = (hipStream_t)c.stream;
  if (wave)
    HIP_TRY(hipMemcpyAsync(w.opd_groups, wave->groups, (size_t)c.n_groups * SENS_OPD_GROUP * sizeof(double), hipMemcpyHostToDevice, st));
  if (w.glass)
    HIP_TRY(hipMemcpyAsync(w.glass, glasses.data(), glasses.size() * sizeof(SensGlass), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(w.words, 0, 64, st));
  HIP_TRY(hipMemsetAsync(w.stamp, 0, (size_t)c.n_ids * sizeof(int), st));
  HIP_TRY(hipMemcpyAsync(w.table, table.data(), table.size() * sizeof(SensSurface), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.first, c.group_first, (size_t)(c.n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.pivots, c.pivots, (size_t)c.n_groups * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  return PRT_OK;
}

// the steps, one launch per generation in order (`launch(grid, start, count, generation)`)
template <class Launch>
static void sens_steps(const SensCall& c, Launch launch) {
  int64_t start = 0;
  for (int g = 0; g < c.n_generations; ++g) {
    const int64_t count = c.rows_per_generation[g];
    if (count) launch(dim3((unsigned)((count + kSensBlock - 1) / kSensBlock)), start, count, g);
    start += count;
  }
}

// the sums: the partials of every group's chunks, folded in a fixed order; the wavefront form's own behind them
static void sens_sums(const SensCall& c, const SensWork& w, const SensOpdCall* wave, int64_t n_rows, int chunks) {
  hipStream_t st = (hipStream_t)c.stream;
  const int K = c.n_parameters, entries = sens_entries(K);
  const dim3 grid((unsigned)chunks, (unsigned)c.n_groups);
  if (chunks)
    hipLaunchKernelGGL(k_sens_partials, grid, dim3(kSensBlock), 0, st, c.rows, c.ld, n_rows, c.selected, c.n_selected,
                       w.first, K, c.weight_column, w.pivots, c.jacobian_out, w.partials, &w.words->status);
  hipLaunchKernelGGL(k_sens_fold, dim3((unsigned)((int64_t)c.n_groups * entries)), dim3(64), 0, st, w.partials, chunks,
                     entries, c.n_groups, c.sums_out);
  if (!wave) return;
  const int opd_entries = sens_opd_entries(K, wave->n_terms);
  const size_t lds = (size_t)SENS_OPD_TILE * sens_opd_stride(K, wave->n_terms) * sizeof(double);
  if (chunks)
    hipLaunchKernelGGL(k_sens_opd_partials, grid, dim3(kSensBlock), lds, st, c.rows, c.ld, n_rows, c.selected,
                       c.n_selected, w.first, K, wave->n_terms, c.weight_column, c.jacobian_out, wave->opd, wave->pupil,
                       wave->dfield, wave->dopd, w.opd_partials, &w.words->status);
  hipLaunchKernelGGL(k_sens_fold, dim3((unsigned)((int64_t)c.n_groups * opd_entries)), dim3(64), 0, st, w.opd_partials,
                     chunks, opd_entries, c.n_groups, wave->sums);
}

// the status words read back: what the kernels refused, and the counters
static int sens_report(const SensCall& c, const SensWork& w) {
  hipStream_t st = (hipStream_t)c.stream;
  SensWords host_words;
  HIP_TRY(hipMemcpyAsync(&host_words, w.words, sizeof(SensWords), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  const int rc = join_refusal(host_words.status, "sensitivity");
  if (rc) return rc;
  if (host_words.status & SENS_BAD_SELECTION)
    return fail(PRT_ERR_ARG, "sensitivity: row_slot or selected points outside the selection or the frame");
  for (int k = 0; k < SENS_COUNTERS; ++k) c.record_out[k] = (int64_t)host_words.count[k];
  return PRT_OK;
}

// A call: the parts that are present choose the form.  None: the rigid form (sens_row<false>, six planes of state);
// `design`: seven planes; `wave` (with design): eight, and the wavefront outputs and sums; `launch` (with design, with or
// without wave): the seeds, the glass table and the slopes.  Everything is checked before a device is touched
static int sens_run(const SensCall& c, const SensDesignCall* design, const SensOpdCall* wave, const SensLaunchCall* launch) {
  int64_t max_group_rows = 0;
  const int64_t n_rows = sens_check(c, design, wave, max_group_rows);
  if (n_rows < 0) return (int)n_rows;
  std::vector<SensSurface> table;
  std::vector<SensGlass> glasses;
  SensArgs args;
  SensDesign shape;
  SensLaunch seed;
  std::memset(&shape, 0, sizeof(shape));
  std::memset(&seed, 0, sizeof(seed));
  int rc = sens_table(c, table);
  if (!rc) rc = sens_rigid(c, args, table);
  if (!rc && design) rc = sens_design(c, *design, shape, table);
  if (!rc && launch) rc = sens_launch(c, *launch, seed, shape, glasses);
  if (rc) return rc;
  const SensSizes sizes = {c.n_ids, c.n_surfaces, c.n_parameters, c.n_groups, max_group_rows};
  if (!sens_sizes_ok(sizes)) return fail(PRT_ERR_ARG, "sensitivity: too many rows in a group");
  for (int k = 0; k < SENS_COUNTERS; ++k) c.record_out[k] = 0;
  rc = ops_device(c.device);
  if (rc) return rc;
  const SensWork w = sens_layout(c.workspace, sizes, wave ? 8 : design ? 7 : 6, wave ? wave->n_terms : 0, launch != nullptr);
  SensOpd field;
  std::memset(&field, 0, sizeof(field));
  if (wave) {
    field.opl = wave->opl; field.groups = w.opd_groups; field.first = w.first; field.n_groups = c.n_groups;
    for (int k = 0; k < 3; ++k) { field.e1[k] = wave->axes[3 + k]; field.e2[k] = wave->axes[6 + k]; }
    field.dfield = wave->dfield; field.dopd = wave->dopd; field.dpupil = wave->dpupil; field.opd = wave->opd;
    field.pupil = wave->pupil;
  }
  rc = sens_upload(c, w, table, glasses, wave);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)c.stream;
  const dim3 block(kSensBlock);
  // the step of the form, chosen once
  if (launch && wave)
    sens_steps(c, [&](dim3 grid, int64_t start, int64_t count, int g) {
      hipLaunchKernelGGL(k_sens_launch_opd_step, grid, block, 0, st, c.rows, c.ld, n_rows, start, count, g, c.id0, c.n_ids,
                         args, shape, field, seed, w.table, w.glass, w.state, w.last_row, w.stamp, w.words, c.row_slot,
                         c.n_selected, c.jacobian_out, launch->slopes);
    });
  else if (launch)
    sens_steps(c, [&](dim3 grid, int64_t start, int64_t count, int g) {
      hipLaunchKernelGGL(k_sens_launch_step, grid, block, 0, st, c.rows, c.ld, n_rows, start, count, g, c.id0, c.n_ids, args,
                         shape, seed, w.table, w.glass, w.state, w.last_row, w.stamp, w.words, c.row_slot, c.n_selected,
                         c.jacobian_out, launch->slopes);
    });
  else if (wave)
    sens_steps(c, [&](dim3 grid, int64_t start, int64_t count, int g) {
      hipLaunchKernelGGL(k_sens_opd_step, grid, block, 0, st, c.rows, c.ld, n_rows, start, count, g, c.id0, c.n_ids, args,
                         shape, field, w.table, w.state, w.last_row, w.stamp, w.words, c.row_slot, c.n_selected,
                         c.jacobian_out);
    });
  else if (design)
    sens_steps(c, [&](dim3 grid, int64_t start, int64_t count, int g) {
      hipLaunchKernelGGL(k_sens_design_step, grid, block, 0, st, c.rows, c.ld, n_rows, start, count, g, c.id0, c.n_ids, args,
                         shape, w.table, w.state, w.last_row, w.stamp, w.words, c.row_slot, c.n_selected, c.jacobian_out);
    });
  else
    sens_steps(c, [&](dim3 grid, int64_t start, int64_t count, int g) {
      hipLaunchKernelGGL(k_sens_step, grid, block, 0, st, c.rows, c.ld, n_rows, start, count, g, c.id0, c.n_ids, args, w.table,
                         w.state, w.last_row, w.stamp, w.words, c.row_slot, c.n_selected, c.jacobian_out);
    });
  sens_sums(c, w, wave, n_rows, (int)sens_chunks(max_group_rows));
  return sens_report(c, w);
}

extern "C" int prt_frame_sensitivity(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                     int n_generations, double id0, int64_t n_ids, const prt_prim* surfaces,
                                     int n_surfaces, const double* twists, const int64_t* parameter_ids,
                                     const int32_t* parameter_first, int n_parameters, const int64_t* row_slot,
                                     const int64_t* selected, int64_t n_selected, const int64_t* group_first,
                                     int n_groups, int weight_column, const double* pivots, double* jacobian_out,
                                     double* sums_out, int64_t* record_out, void* workspace, void* stream) {
  const SensCall call = {device, rows, ld, rows_per_generation, n_generations, id0, n_ids, surfaces, n_surfaces, twists,
                         parameter_ids, parameter_first, n_parameters, row_slot, selected, n_selected, group_first,
                         n_groups, weight_column, pivots, jacobian_out, sums_out, record_out, workspace, stream};
  return sens_run(call, nullptr, nullptr, nullptr);
}

extern "C" int prt_frame_design_sensitivity(int device, const double* rows, int64_t ld,
                                            const int64_t* rows_per_generation, int n_generations, double id0,
                                            int64_t n_ids, const prt_prim* surfaces, int n_surfaces, const double* twists,
                                            const int64_t* parameter_ids, const int32_t* parameter_first,
                                            const double* linear, const double* index_rates, const int64_t* index_ids,
                                            const int32_t* index_first, int n_parameters, const int64_t* row_slot,
                                            const int64_t* selected, int64_t n_selected, const int64_t* group_first,
                                            int n_groups, int weight_column, const double* pivots, double* jacobian_out,
                                            double* sums_out, int64_t* record_out, void* workspace, void* stream) {
  const SensCall call = {device, rows, ld, rows_per_generation, n_generations, id0, n_ids, surfaces, n_surfaces, twists,
                         parameter_ids, parameter_first, n_parameters, row_slot, selected, n_selected, group_first,
                         n_groups, weight_column, pivots, jacobian_out, sums_out, record_out, workspace, stream};
  const SensDesignCall design = {linear, index_rates, index_ids, index_first};
  return sens_run(call, &design, nullptr, nullptr);
}

extern "C" int prt_frame_opd_sensitivity(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                         int n_generations, double id0, int64_t n_ids, const prt_prim* surfaces,
                                         int n_surfaces, const double* twists, const int64_t* parameter_ids,
                                         const int32_t* parameter_first, const double* linear, const double* index_rates,
                                         const int64_t* index_ids, const int32_t* index_first, int n_parameters,
                                         const int64_t* row_slot, const int64_t* selected, int64_t n_selected,
                                         const int64_t* group_first, int n_groups, int weight_column, const double* pivots,
                                         const double* opl, const double* wavefront_groups, const double* axes, int n_terms,
                                         double* jacobian_out, double* sums_out, double* dfield_out, double* dopd_out,
                                         double* dpupil_out, double* opd_out, double* pupil_out, double* opd_sums_out,
                                         int64_t* record_out, void* workspace, void* stream) {
  const SensCall call = {device, rows, ld, rows_per_generation, n_generations, id0, n_ids, surfaces, n_surfaces, twists,
                         parameter_ids, parameter_first, n_parameters, row_slot, selected, n_selected, group_first,
                         n_groups, weight_column, pivots, jacobian_out, sums_out, record_out, workspace, stream};
  const SensDesignCall design = {linear, index_rates, index_ids, index_first};
  const SensOpdCall wave = {opl, wavefront_groups, axes, n_terms, dfield_out, dopd_out, dpupil_out, opd_out, pupil_out,
                            opd_sums_out};
  return sens_run(call, &design, &wave, nullptr);
}

// (opl == NULL: the launch form without the wavefront)
extern "C" int prt_frame_launch_sensitivity(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                            int n_generations, double id0, int64_t n_ids, const prt_prim* surfaces,
                                            int n_surfaces, const double* twists, const int64_t* parameter_ids,
                                            const int32_t* parameter_first, const double* linear, const double* index_rates,
                                            const int64_t* index_ids, const int32_t* index_first, int n_parameters,
                                            const int64_t* row_slot, const int64_t* selected, int64_t n_selected,
                                            const int64_t* group_first, int n_groups, int weight_column,
                                            const double* pivots, const double* opl, const double* wavefront_groups,
                                            const double* axes, int n_terms, const double* launch_ranges,
                                            const int32_t* launch_flags, const double* wavelength_rates,
                                            const prt_material* materials, int n_materials, double* jacobian_out,
                                            double* sums_out, double* slopes_out, double* dfield_out, double* dopd_out,
                                            double* dpupil_out, double* opd_out, double* pupil_out, double* opd_sums_out,
                                            int64_t* record_out, void* workspace, void* stream) {
  const SensCall call = {device, rows, ld, rows_per_generation, n_generations, id0, n_ids, surfaces, n_surfaces, twists,
                         parameter_ids, parameter_first, n_parameters, row_slot, selected, n_selected, group_first,
                         n_groups, weight_column, pivots, jacobian_out, sums_out, record_out, workspace, stream};
  const SensDesignCall design = {linear, index_rates, index_ids, index_first};
  const SensOpdCall wave = {opl, wavefront_groups, axes, n_terms, dfield_out, dopd_out, dpupil_out, opd_out, pupil_out,
                            opd_sums_out};
  const SensLaunchCall launch = {launch_ranges, launch_flags, wavelength_rates, materials, n_materials, slopes_out};
  return sens_run(call, &design, opl ? &wave : nullptr, &launch);
}

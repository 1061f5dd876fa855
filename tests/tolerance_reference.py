"""An extended-precision reference of the tolerancing pass (prt_frame_tolerance and prt_frame_tolerance_moments: the
definitions of include/prt.h), the error budget the kernels of prt_tolerance.hpp are held to, Python copies of their
partition rules and the inputs the tests run on.  It builds on tests/diffraction_reference.py (``phasor``,
``inverse_wavelength``, EPS_TRIG, F32_TURN) and tests/psf_gradient_reference.py (``gradient_case``) and changes nothing
there.

The formulas, per group g and wavelength l (s = 1 / lambda_w), over the rays kept, C columns x_c, trial m with p_c:
    a = sqrt(w),  c0 = OPD s,  e_c = x_c s,  phi_m = c0 + sum_c e_c p_c   (cycles)
    U_lm = s sum a exp(2 pi i phi_m),  Strehl_m = sum_l |U_lm|^2 / D_g,  D_g = sum_l (s_l sum a)^2
A ray is kept if its OPD is finite, its weight finite and >= 0 and all C column values finite.
Moments, per group over the kept rays of every wavelength, v = (1, OPD, x_1 .. x_C): sum w v_i v_j.

What counts as an input: opd, the columns, the trial values, the weight and wavelength columns, 1 / lambda_w as the
library forms it.

The budget, u = 2^-53.
  Per (ray, trial) the device's phase is fma(e_C, p_C, ... fma(e_1, p_1, c0)) with c0 = fl(OPD s), e_c = fl(x_c s).
  Counted, each rounding relative to the magnitude it acts on, B = |c0| + sum_c |e_c p_c|: c0's product 1 of |c0|; e_c's
  product 1 of |e_c p_c|; each of the C fmas 1 of a partial sum that is at most B: (C + 1) u B, and one more of B for
  the terms of second order: (C + 2) u B cycles.  v_fract_f64 is exact; the conversion of the turn to float moves it by
  at most F32_TURN; (v_cos_f32, v_sin_f32) are within EPS_TRIG of the unit phasor.  With |exp(ia) - exp(ib)| <= |a - b|:
      eps_rm = EPS_TRIG + 2 pi F32_TURN + 2 pi u (C + 2) B_rm
      |U~_lm - U_lm| <= s sum_r a_r eps_rm =: A_lm
      |Strehl~_m - Strehl_m| <= sum_l (2 |U_lm| A_lm + A_lm^2) / D_g + (2 depth + 10) u Strehl_m
  the last term for sum a (a tree and the slices, ``depth`` additions), the squares, the sum and the division, as
  ``strehl_eta`` of diffraction_reference counts them.  What the budget leaves to EPS_TRIG's margin, as the PSF's does:
  the fp64 accumulation of the phasor sums (at most rays-per-slice + slices times u of sum a).
  Moments: entry (i, j) is sum_r fma(fl(w v_i), v_j, acc) over the rows of a chunk in order, the chunks then added in
  order.  A term passes one rounding for w v_i, at most n_c fmas (n_c = the rows of its chunk, at most kTolMomentChunk)
  and at most ``chunks`` additions of the fold: |S~ - S| <= gamma_n sum |w v_i v_j|, n = 1 + min(rows, kTolMomentChunk)
  + chunks, gamma_n = n u / (1 - n u).  The counts are integers and exact.
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

import diffraction_reference as R
import psf_gradient_reference as G

LD = R.LD
MAX_COLUMNS, MAX_TRIALS = 20, 65536


def kernel_constants():
    """The static const ints of prt_tolerance.hpp (kTolTrials, kTolTile, kTolRays, ...)."""
    found = dict(vars(R.K))
    text = open(os.path.join(R.ROOT, "pyrayt_amd", "csrc", "prt_tolerance.hpp")).read()
    for key, value in re.findall(r"static const (?:int|size_t) (k\w+) = ([^;]+);", text):
        value = re.sub(r"(\d+)u\b", r"\1", value)
        try:
            found[key] = int(eval(value, {"__builtins__": {}}, dict(found)))
        except (NameError, SyntaxError, TypeError):
            pass  # (not a plain constant)
    return SimpleNamespace(**found)


K = kernel_constants()
# Python copies of lines of prt_frame_tolerance and of psf_plan as it calls it, held to the headers' text by
# tests/test_host_tolerance.py
HOST_RULES = {
    "prt_tolerance.hpp": (
        "enum { TOL_MAX_COLUMNS = 20, TOL_MAX_TRIALS = 65536, TOL_RECORD = 5, TOL_BAD_WAVELENGTH = 1, TOL_BAD_ROW = 2 };",
        "static_assert(kTolMinSlice == kPsfMinSlice,",
        "PsfPlan plan = psf_plan(cus, n_selected, buckets, buckets, 1, 1, 16, 0, 1);",
        "int64_t chunk = (int64_t)(kPsfSlabBytes / ((size_t)buckets * slices * 16)) / kTolTile * kTolTile;",
        "for (int64_t base = lo; base < hi; base += kTolRays) {",
        "const int64_t chunks = (group_first[g + 1] - group_first[g] + kTolMomentChunk - 1) / kTolMomentChunk;",
        "trial_columns<TOL_MAX_COLUMNS>(C, sum, first, n);"),
    "prt_trials.hpp": (  # (the instantiation and the launches, as prt_frame_tolerance calls them)
        'static_assert(MAX == 16 || MAX == 20, "the ladder ends at 16 or at 20 columns");',
        "else if (MAX == 16 || K <= 16) launch(std::integral_constant<int, 16>(), more...);",
        "else if constexpr (MAX == 20) launch(std::integral_constant<int, 20>(), more...);",
        "for (int first = 0; first < M; first += (int)most) launch(first, M - first < most ? M - first : (int)most);"),
    "prt_psf.hpp": G.HOST_RULES["prt_psf.hpp"],
}


def slices(n_selected, buckets, cus):
    """The ray slices prt_frame_tolerance picks (psf_plan for one pixel): they follow the selection's size, the buckets
    and the CUs, never n_rows, M or C."""
    s = (4 * cus + buckets - 1) // buckets
    s = min(s, max(1, n_selected // (buckets * K.kTolMinSlice)))
    s = min(s, K.kPsfSlabBytes // (buckets * 16))
    return max(1, min(s, K.kPsfMaxSlices))


def trial_chunk(buckets, n_slices):
    """The trials of one k_tol_sum launch at most."""
    return K.kPsfSlabBytes // (buckets * n_slices * 16) // K.kTolTile * K.kTolTile


def template_columns(n_columns):
    """The instantiation k_tol_sum<CP> that serves C columns."""
    return -(-n_columns // K.kTolColumnStep) * K.kTolColumnStep


# ---- the reference --------------------------------------------------------------------------------------------------------
def tolerance_inputs(group, wavelength, opd, weight, columns, wavelengths, unit, n_groups):
    """The pass's inputs, one entry per selected row in the selection's order (fp64): group, wavelength (um), opd,
    weight, columns (C, n); the distinct wavelengths, world_unit_um."""
    f = lambda x: np.asarray(x, dtype=np.float64)  # noqa: E731
    return SimpleNamespace(group=np.asarray(group, dtype=np.int64), wavelength=f(wavelength), opd=f(opd), weight=f(weight),
                           columns=np.atleast_2d(f(columns)), wavelengths=f(wavelengths), unit=float(unit),
                           n_groups=int(n_groups))


def kept_rays(inp):
    """(passes the PSF's rule, every column finite), per ray."""
    usable = np.isfinite(inp.opd) & (inp.weight >= 0) & np.isfinite(inp.weight)
    return usable, np.all(np.isfinite(inp.columns), axis=0)


def tolerance_reference(inp, trials, n_slices=1):
    """The formulas of the module docstring on ``inp`` and ``trials`` (G, M, C).  A namespace, G groups, L wavelengths, M
    trials, longdouble: amplitude (re, im) (G, L, M), strehl (G, M); float64: amplitude_bound, strehl_bound; record
    (G, L, 5) longdouble; n_rays, n_missed, n_unfollowed (G, L).  A group without kept rays is NaN."""
    trials = np.asarray(trials, dtype=np.float64)
    n_groups, L = inp.n_groups, len(inp.wavelengths)
    M, C = trials.shape[1], trials.shape[2]
    assert trials.shape[0] == n_groups and C == len(inp.columns)
    nan = lambda *shape, dtype=LD: np.full(shape, np.nan, dtype=dtype)  # noqa: E731
    are, aim, abound = nan(n_groups, L, M), nan(n_groups, L, M), nan(n_groups, L, M, dtype=float)
    strehl, strehl_bound = nan(n_groups, M), nan(n_groups, M, dtype=float)
    record = np.zeros((n_groups, L, 5), dtype=LD)
    n_rays, n_missed, n_unfollowed = (np.zeros((n_groups, L), dtype=np.int64) for _ in range(3))
    usable, followed = kept_rays(inp)
    for g in range(n_groups):
        parts = []
        for l, lam in enumerate(inp.wavelengths):
            mine = (inp.group == g) & (inp.wavelength == lam)
            m = mine & usable & followed
            n = int(m.sum())
            n_rays[g, l], n_missed[g, l] = n, int((mine & ~usable).sum())
            n_unfollowed[g, l] = int((mine & usable & ~followed).sum())
            s = R.inverse_wavelength(lam, inp.unit)
            S = LD(s)
            a = np.sqrt(inp.weight[m])
            A = a.astype(LD)
            opd, x = inp.opd[m].astype(LD), inp.columns[:, m].astype(LD)  # (n), (C, n)
            re, im, err = np.zeros(M, dtype=LD), np.zeros(M, dtype=LD), np.zeros(M)
            c0_abs = np.abs(inp.opd[m] * s)
            e_abs = np.abs(inp.columns[:, m] * s)
            for lo, hi in R._chunks(M, max(1, n * (C + 2))):
                p = trials[g, lo:hi].astype(LD)                                  # (m, C)
                cs, sn = R.phasor((opd[None, :] + p @ x) * S)
                re[lo:hi], im[lo:hi] = (A * cs).sum(axis=1), (A * sn).sum(axis=1)
                size = c0_abs[None, :] + np.abs(trials[g, lo:hi]) @ e_abs        # B_rm
                eps = R.EPS_TRIG + 2 * math.pi * R.F32_TURN + 2 * math.pi * R.U64 * (C + 2) * size
                err[lo:hi] = (a[None, :] * eps).sum(axis=1)
            sum_a = A.sum()
            record[g, l] = (n, n_missed[g, l], n_unfollowed[g, l], sum_a, (S * sum_a) ** 2)
            parts.append(SimpleNamespace(s=s, re=re, im=im, err=err, sum_a=sum_a, rays=n))
        den = sum((LD(p.s) * p.sum_a) ** 2 for p in parts)
        if not n_rays[g].sum() or not den > 0:
            continue
        strehl[g], strehl_bound[g] = 0, 0
        for l, p in enumerate(parts):
            S = LD(p.s)
            are[g, l], aim[g, l] = S * p.re, S * p.im
            abound[g, l] = p.s * p.err
            part = (are[g, l] ** 2 + aim[g, l] ** 2) / den
            depth = -(-(-(-max(p.rays, 1) // n_slices)) // K.kPsfBlock) + int(math.log2(K.kPsfBlock)) + n_slices
            size_u = np.hypot(are[g, l], aim[g, l]).astype(float)
            strehl[g] += part
            strehl_bound[g] += ((2 * size_u * abound[g, l] + abound[g, l] ** 2) / float(den)
                                + (2 * depth + 10) * R.U64 * part.astype(float))
    return SimpleNamespace(amplitude=(are, aim), amplitude_bound=abound, strehl=strehl, strehl_bound=strehl_bound,
                           record=record, n_rays=n_rays, n_missed=n_missed, n_unfollowed=n_unfollowed)


def gamma(n):
    return n * R.U64 / (1 - n * R.U64)


def moments_reference(inp):
    """(moments, bound): (G, 3 + (C + 2)(C + 3) / 2) longdouble and float64, the layout of include/prt.h."""
    C = len(inp.columns)
    width = 3 + (C + 2) * (C + 3) // 2
    out, bound = np.zeros((inp.n_groups, width), dtype=LD), np.zeros((inp.n_groups, width))
    usable, followed = kept_rays(inp)
    listed = np.isin(inp.wavelength, inp.wavelengths)
    tri = np.tril_indices(C + 1)
    for g in range(inp.n_groups):
        mine = (inp.group == g) & listed
        m = mine & usable & followed
        out[g, :3] = (int(m.sum()), int((mine & ~usable).sum()), int((mine & usable & ~followed).sum()))
        w = inp.weight[m].astype(LD)
        y = np.vstack([inp.opd[m][None, :], inp.columns[:, m]]).astype(LD)        # (C + 1, n)
        rows = int((inp.group == g).sum())
        chunks = -(-rows // K.kTolMomentChunk)
        g_n = gamma(1 + min(rows, K.kTolMomentChunk) + chunks)
        second = (w[None, None, :] * y[:, None, :] * y[None, :, :])
        out[g, 3], bound[g, 3] = w.sum(), g_n * float(np.abs(w).sum())
        out[g, 4:5 + C] = (w[None, :] * y).sum(axis=1)
        bound[g, 4:5 + C] = g_n * np.abs(w[None, :] * y).sum(axis=1).astype(float)
        out[g, 5 + C:] = second.sum(axis=2)[tri]
        bound[g, 5 + C:] = g_n * np.abs(second).sum(axis=2)[tri].astype(float)
    return out, bound


def rms_opd_reference(inp, q):
    """(G, M) longdouble: the weighted sample statistic (piston removed) of OPD + sum_c q_gmc x_c over the kept rays of
    the group, every wavelength together.  ``q``: (G, M, C)."""
    usable, followed = kept_rays(inp)
    out = np.full(q.shape[:2], np.nan, dtype=LD)
    for g in range(inp.n_groups):
        m = (inp.group == g) & usable & followed & np.isin(inp.wavelength, inp.wavelengths)
        w = inp.weight[m].astype(LD)
        if not w.sum() > 0:
            continue
        moved = inp.opd[m].astype(LD)[None, :] + np.asarray(q[g], dtype=np.float64).astype(LD) @ inp.columns[:, m].astype(LD)
        mean = (moved * w).sum(axis=1) / w.sum()
        out[g] = np.sqrt(((moved - mean[:, None]) ** 2 * w).sum(axis=1) / w.sum())
    return out


def deviation(got, re, im=None):
    return G.deviation(got, re, im)


# ---- the inputs of the tests (CPU and GPU) ----------------------------------------------------------------------------------
def tolerance_case(counts, n_columns, **kw):
    """``psf_gradient_reference.gradient_case`` with ``n_columns`` parameters (its dopd are the columns: about a wave per
    unit, smooth over the pupil plus noise) and, on top, ``inputs()``: the ``tolerance_inputs`` of its selected rows."""
    case = G.gradient_case(counts, n_columns, **kw)
    base = case.inputs(np.zeros(1), np.zeros(1))

    def inputs(columns=None, weight=None):
        return tolerance_inputs(base.group, base.wavelength, base.opd, base.weight if weight is None else weight,
                                case.dopd if columns is None else columns, base.wavelengths, base.unit, case.n_groups)

    case.tolerance_inputs = inputs
    return case


def random_trials(n_groups, n_trials, n_columns, scale=0.4, seed=1):
    """(G, M, C) trial values of about ``scale`` (the case's columns move the OPD by about a wave per unit)."""
    return np.random.default_rng(seed).uniform(-scale, scale, (n_groups, n_trials, n_columns))


SIZES = G.SIZES
# M as the caller gives it; ``tolerance`` appends the nominal trial, so the kernel runs M + 1: both M and M + 1 take every
# value about the trials of a thread and of a workgroup (T - 1 .. T + 1, tile - 1 .. tile + 1) and 1 025.  The kernel's own
# n_trials = 1 is a direct call of the entry point (tests/test_gpu_tolerance.py)
TRIAL_COUNTS = tuple(sorted({1, K.kTolTrials - 1, K.kTolTrials, K.kTolTrials + 1, K.kTolTile - 2, K.kTolTile - 1, K.kTolTile,
                             K.kTolTile + 1, 1024, 1025} - {0}))
COLUMN_COUNTS = (1, 3, 4, 5, 16, 19, 20)

"""An extended-precision reference of the Monte Carlo tolerancing of the geometric MTF (the definitions of include/prt.h
under prt_frame_mtf_tolerance: the moments and the OTF per trial), the error budget k_mtft_moments, k_mtft_focus and
k_mtft_sum are held to, Python copies of the new partition rules and the inputs the tests run on.  It builds on
tests/mtf_gradient_reference.py (the staged quantities, their counted roundings and its case builders) and on
tests/diffraction_reference.py (the phasor, EPS_TRIG) and changes nothing there.

What counts as an input: the frame's rows, ``jacobian`` and ``slopes`` (exact, whatever pass made them), the trials, the
(kc, ks) table as the library's host code forms it, the centre C_g the device used and, where the focus is compensated,
the focus shift delta_m the device applied (held to ``best_focus_bound`` on its own).

The staged values, from mtf_gradient_reference's count (u = 2^-53, each relative to its magnitude): p within 10 P, s
within 4 S, dp_k within 24 DP_k, ds_k within 17 DS_k.  A trial of K parameters moves a ray by the chains
    P = fma(t_K, dp_K, ... fma(t_1, dp_1, p)),  S likewise:  K roundings, each of at most the chain's magnitude
    MP = P + sum_k |t_k| DP_k  and  MS = S + sum_k |t_k| DS_k  (capital P, S on the right the magnitudes of the staged ones):
  P within (24 + K) u MP, S within (17 + K) u MS (columns past K are zeros and round nothing).  The plane of the trial,
    X = fma(delta_m, S, P): one rounding more, X within (25 + K) u MX, MX = MP + |delta_m| MS.
  The phase fma(kc, X1, fma(ks, X2, fma(kc delta_f, S1, (ks delta_f) S2))): one rounding for each of kc delta_f and
    ks delta_f, one for the innermost product and one per fma: the X terms carry 25 + K + 2, the S terms
    17 + K + 1 + 1 + 3 = 22 + K.  27 + K, and one more for the terms of second order:
    K_T(K) = 28 + K roundings of T_r = |kc| MX1 + |ks| MX2 + |delta_f| (|kc| MS1 + |ks| MS2).
  These are the (4 K + 2)-term chains of a ray and trial: 4 K multiply-adds of the move, 2 of the plane.
The budget per output and trial (``otf_bound``), with the MTF's phasor budget over the moved ray:

    |OTF~ - OTF| <= mean_w(e_r),   e_r = EPS_TRIG + (2 pi 2^-25)^2 / 2 + 2 pi K_T(K) u T_r

  What it leaves to EPS_TRIG's margin, as the OTF's does: c' = fma(-theta, sn, c) and the accumulation fma(w, c', re)
  (at most rays-per-slice times u of sum w) and the normalisation.
The moments (``moments_bound``), a gamma_n-type bound: a sum over n rays added one after another and then over the
  slices rounds at most n + slices times, each product under it a few times; with c = 2 (24 + K) + 4 + n + 256
    |sum~ - sum| <= gamma_c sum_r w M_r,  gamma_c = c u / (1 - c u),
  M_r the magnitude of the ray's term (1; MP; MS; MP.MP; MP.MS; MS.MS) -- the squares carry both factors' roundings,
  2 (24 + K), the products w x and the two fmas 4.  n is the group's count of selected rows: no slice is longer.
The least-squares focus (``best_focus_bound``): delta* = -cov / var with cov = m6 / m0 - mean P . mean S and
  var = m7 / m0 - |mean S|^2 carries the moments' bounds B_q to first order, the quotient rule term by term, plus the
  8 roundings of k_mtft_focus's own arithmetic on the same magnitudes:
    E_cov = (B6 + B0 |m6| / m0) / m0 + sum_i [(B_Pi + B0 |mean P_i|) |mean S_i| + |mean P_i| (B_Si + B0 |mean S_i|)] / m0
            + 8 u (|m6| / m0 + sum_i |mean P_i mean S_i|),   E_var likewise with S for P,
    |delta~ - delta*| <= (E_cov + |delta*| E_var) / (var - E_var)   (infinite where var <= E_var).
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

import diffraction_reference as R
import mtf_gradient_reference as G

LD = R.LD
MAX_PARAMETERS = 16
K_P, K_S = 24, 17  # (the staged dp and ds, and with them the chains P and S, before the chain's own K roundings)


def k_t(n_parameters):
    return 28 + n_parameters


def kernel_constants():
    """The static const ints of prt_mtf_tolerance.hpp (kMtftBlock, kMtftTile, ...), after those of prt_mtf.hpp."""
    found = {}
    for name in ("prt_mtf.hpp", "prt_mtf_tolerance.hpp"):
        text = open(os.path.join(R.ROOT, "pyrayt_amd", "csrc", name)).read()
        for key, value in re.findall(r"static const (?:int|size_t) (k\w+) = ([^;]+);", text):
            value = re.sub(r"(\d+)u\b", r"\1", value)
            try:
                found[key] = int(eval(value, {"__builtins__": {}}, dict(found)))
            except (NameError, SyntaxError, TypeError):
                pass  # (not a plain constant)
    return SimpleNamespace(**found)


K = kernel_constants()
# Python copies of lines of prt_frame_mtf_tolerance and of mtf_slices (prt_mtf.hpp) as it calls it, held to the headers'
# text by tests/test_host_mtf_tolerance.py
HOST_RULES = {
    "prt_mtf_tolerance.hpp": (
        "enum { MTFT_MAX_TRIALS = 65536, MTFT_RECORD = 7, MTFT_MOMENTS = 8 };",
        "static const int kMtftTile = kMtftBlock * kMtftTrials;",
        "const int64_t s = ((int64_t)kMtftSlicesPerCu * cus + n_groups - 1) / n_groups;",
        "return s < 1 ? 1 : (s > kMtfMaxSlices ? kMtfMaxSlices : s);",
        "const MtfgStaging staging(group_first, n_groups, K, mtft_max_slices(cus, n_groups), workspace);",
        "const int64_t n_out = plan.n_out, all_outputs = (n_out + kMtftOut - 1) / kMtftOut * kMtftOut;",
        "const int64_t tile_room = (int64_t)(kMtftSlabBytes / ((size_t)slice_grid * kMtftTile)) - MTFT_MOMENTS * 8;",
        "const int64_t outputs = std::min<int64_t>(all_outputs, tile_room / 16 / kMtftOut * kMtftOut);",
        "if (outputs < kMtftOut) return fail(PRT_ERR_ARG, cap);",
        "const size_t trial_bytes = (size_t)slice_grid * (MTFT_MOMENTS * 8 + (size_t)outputs * 16);",
        "int64_t most = (int64_t)(kMtftSlabBytes / trial_bytes) / kMtftTile * kMtftTile;",
        "most = std::min<int64_t>(most, ((int64_t)M + kMtftTile - 1) / kMtftTile * kMtftTile);",
        "trial_launches(M, most, [&](int first, int n) { trial_columns<MTFG_MAX_PARAMETERS>(K, launch, first, n); });",
        "for (int64_t base = lo; base < hi; base += kMtftRays) {"),
    "prt_trials.hpp": (  # (the ladder and the loop over the launches, as prt_frame_mtf_tolerance calls them)
        'static_assert(MAX == 16 || MAX == 20, "the ladder ends at 16 or at 20 columns");',
        "if (K <= 4) launch(std::integral_constant<int, 4>(), more...);",
        "else if (K <= 8) launch(std::integral_constant<int, 8>(), more...);",
        "else if (K <= 12) launch(std::integral_constant<int, 12>(), more...);",
        "else if (MAX == 16 || K <= 16) launch(std::integral_constant<int, 16>(), more...);",
        "for (int first = 0; first < M; first += (int)most) launch(first, M - first < most ? M - first : (int)most);"),
    "prt_mtf_gradient.hpp": (  # (the staging's slices, cut by the limit this pass hands it)
        "h_slice[g + 1] = h_slice[g] + mtf_slices(count, max_slices);",),
    "prt_mtf.hpp": (
        "const int64_t s = (count + kMtfMinSlice - 1) / kMtfMinSlice;",
        "return s < 1 ? 1 : (s > max_slices ? max_slices : s);"),
}


def max_slices(cus, n_groups):
    return min(max(-(-K.kMtftSlicesPerCu * cus // n_groups), 1), K.kMtfMaxSlices)


def slices(count, n_groups, cus):
    """The ray slices of a group of ``count`` selected rows: they follow nothing but count, n_groups and the CU count."""
    return min(max(-(-count // K.kMtfMinSlice), 1), max_slices(cus, n_groups))


def launches(total_slices, n_out, n_trials):
    """(outputs, trials) of a launch at most: whole chunks of outputs, as many as one tile of trials leaves room for under
    the slab cap, then whole tiles of trials; None where not even a chunk fits (the call is refused)."""
    every = -(-n_out // K.kMtftOut) * K.kMtftOut
    outputs = min(every, (K.kMtftSlabBytes // (total_slices * K.kMtftTile) - 8 * 8) // 16 // K.kMtftOut * K.kMtftOut)
    if outputs < K.kMtftOut:
        return None
    most = K.kMtftSlabBytes // (total_slices * (8 * 8 + outputs * 16)) // K.kMtftTile * K.kMtftTile
    return outputs, min(most, -(-n_trials // K.kMtftTile) * K.kMtftTile)


def template_columns(n_parameters):
    return -(-n_parameters // K.kMtftColumnStep) * K.kMtftColumnStep


# ---- the reference --------------------------------------------------------------------------------------------------------
def staged(q, u, w, group, n_groups, jacobian, slopes, axes=None, centre=None):
    """Per group the kept rays' staged quantities in longdouble, as mtf_gradient_reference forms them: a list of
    namespaces (None for a group without kept rays or weight) of W, p (2, n), s (2, n), dp, ds (K, 2, n) and the magnitudes
    P, S (2, n), DP, DS (K, 2, n) in float64; and the record (centre, centroid, sum_weights, n_rays, n_missed,
    n_unfollowed)."""
    axes = R.default_axes() if axes is None else np.asarray(axes, dtype=np.float64)
    q, u, w = (np.asarray(x, dtype=np.float64) for x in (q, u, w))
    jacobian, slopes = np.asarray(jacobian, dtype=np.float64), np.asarray(slopes, dtype=np.float64)
    n_par = len(jacobian)
    passes = R.mtf_kept(q, u, w, axes)
    followed = np.all(np.isfinite(jacobian), axis=(0, 1)) & np.all(np.isfinite(slopes), axis=(0, 1))
    a, e1, e2 = (axes[k:k + 3].astype(LD) for k in (0, 3, 6))
    mag = G._magnitude
    centres, centroids, sums = (np.full(shape, np.nan, dtype=LD) for shape in ((n_groups, 3), (n_groups, 3), (n_groups,)))
    used, missed, unfollowed = (np.zeros(n_groups, dtype=np.int64) for _ in range(3))
    out = []
    for g in range(n_groups):
        mine = group == g
        m = mine & passes & followed
        used[g], missed[g], unfollowed[g] = int(m.sum()), int((mine & ~passes).sum()), int((mine & passes & ~followed).sum())
        out.append(None)
        if not used[g]:
            continue
        Q, Uv, W = q[m].astype(LD), u[m].astype(LD), w[m].astype(LD)
        with np.errstate(invalid="ignore", divide="ignore"):  # (a group of zero weights)
            own, _ = R.centroid(q[m], w[m])
        centroids[g] = own
        c = own if centre is None else np.asarray(centre[g], dtype=np.float64).astype(LD)
        centres[g] = c
        sums[g] = W.sum()
        if not sums[g] > 0:
            continue
        d = Q - c
        ua = (Uv @ a) / np.sqrt((Uv * Uv).sum(axis=1))
        s = [(Uv @ e) / (Uv @ a) for e in (e1, e2)]
        da = d @ a
        p = [d @ e - si * da for e, si in zip((e1, e2), s)]
        S = [(mag(Uv, e) + np.abs(si) * mag(Uv, a)) / np.abs(Uv @ a) for e, si in zip((e1, e2), s)]
        P = [mag(d, e) + Si * mag(d, a) for e, Si in zip((e1, e2), S)]
        kappa = mag(Uv, a) / np.abs(Uv @ a)
        dp, ds, DP, DS = ([] for _ in range(4))
        for k in range(n_par):
            dQ, dU = jacobian[k][:, m].T.astype(LD), slopes[k][:, m].T.astype(LD)
            dua, dqa = dU @ a, dQ @ a
            dsk = [(dU @ e - si * dua) / ua for e, si in zip((e1, e2), s)]
            DSk = [(mag(dU, e) + Si * mag(dU, a)) * kappa / np.abs(ua) for e, Si in zip((e1, e2), S)]
            ds.append(dsk)
            DS.append(DSk)
            dp.append([dQ @ e - si * dqa - dsi * da for e, si, dsi in zip((e1, e2), s, dsk)])
            DP.append([mag(dQ, e) + Si * mag(dQ, a) + DSi * mag(d, a) for e, Si, DSi in zip((e1, e2), S, DSk)])
        f64 = lambda x: np.asarray(x, dtype=LD).astype(np.float64)  # noqa: E731
        out[g] = SimpleNamespace(W=W, p=np.asarray(p, dtype=LD), s=np.asarray(s, dtype=LD), dp=np.asarray(dp, dtype=LD),
                                 ds=np.asarray(ds, dtype=LD), P=f64(P), S=f64(S), DP=f64(DP), DS=f64(DS),
                                 n_selected=int(mine.sum()))
    record = SimpleNamespace(centre=centres, centroid=centroids, sum_weights=sums, n_rays=used, n_missed=missed,
                             n_unfollowed=unfollowed, n_parameters=n_par)
    return out, record


def best_focus(moments, bounds=None):
    """delta* = -cov(P, S) / var(S) of (..., 8) longdouble moments (0 where var(S) is not > 0, NaN without weight), and
    with the moments' ``bounds`` the bound of the docstring."""
    m = np.asarray(moments, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        sw = np.where(m[..., 0] > 0, m[..., 0], np.nan)
        mp, ms = m[..., 1:3] / sw[..., None], m[..., 3:5] / sw[..., None]
        cov = m[..., 6] / sw - (mp * ms).sum(axis=-1)
        var = m[..., 7] / sw - (ms * ms).sum(axis=-1)
        delta = np.where(var > 0, -cov / np.where(var > 0, var, 1), np.where(np.isnan(sw), np.nan, 0))
        if bounds is None:
            return delta
        B = np.asarray(bounds, dtype=LD)
        amp, ams = np.abs(mp), np.abs(ms)
        bp, bs = (B[..., 1:3] + B[..., 0, None] * amp) / sw[..., None], (B[..., 3:5] + B[..., 0, None] * ams) / sw[..., None]
        e_cov = ((B[..., 6] + B[..., 0] * np.abs(m[..., 6]) / sw) / sw + (bp * ams + amp * bs).sum(axis=-1)
                 + 8 * R.U64 * (np.abs(m[..., 6]) / sw + (amp * ams).sum(axis=-1)))
        e_var = ((B[..., 7] + B[..., 0] * np.abs(m[..., 7]) / sw) / sw + 2 * (bs * ams).sum(axis=-1)
                 + 8 * R.U64 * (np.abs(m[..., 7]) / sw + (ams * ams).sum(axis=-1)))
        bound = np.where(var > e_var, (e_cov + np.abs(delta) * e_var) / np.where(var > e_var, var - e_var, 1), np.inf)
    return delta, bound.astype(np.float64)


def tolerance_reference(q, u, w, group, n_groups, jacobian, slopes, trials, frequencies, azimuths=(0.0, 90.0),
                        focus=(0.0,), axes=None, centre=None, compensate=False, focus_shift=None):
    """The definitions of include/prt.h from the selected rows in their order and jacobian, slopes (K, 3, n); ``trials``
    (M, K) for every group or (G, M, K).  A namespace of re, im (G, M, F, A, N) longdouble (the OTF about the held
    centre) and otf_bound; moments (G, M, 8) longdouble and moments_bound; best_focus (G, M) and best_focus_bound;
    focus_shift (G, M), what the OTF was taken at: ``focus_shift`` where given (the device's), else best_focus with
    ``compensate`` and 0 without; and the record's fields."""
    rays, rec = staged(q, u, w, group, n_groups, jacobian, slopes, axes, centre)
    n_par = rec.n_parameters
    t = np.asarray(trials, dtype=np.float64)
    t = np.broadcast_to(t[None], (n_groups,) + t.shape) if t.ndim == 2 else t
    M = t.shape[1]
    kc, ks = R.frequency_table(frequencies, azimuths)
    planes = np.asarray(focus, dtype=np.float64)
    F, (A, N) = len(planes), kc.shape
    KC, KS = kc.astype(LD).reshape(-1, 1), ks.astype(LD).reshape(-1, 1)
    aKC, aKS = np.abs(kc).reshape(-1, 1), np.abs(ks).reshape(-1, 1)
    nan = lambda *shape, dtype=LD: np.full(shape, np.nan, dtype=dtype)  # noqa: E731
    re, im, otf_bound = nan(n_groups, M, F, A, N), nan(n_groups, M, F, A, N), nan(n_groups, M, F, A, N, dtype=float)
    moments, moments_bound = nan(n_groups, M, 8), nan(n_groups, M, 8, dtype=float)
    moved = [None] * n_groups
    for g, ray in enumerate(rays):
        if ray is None:
            continue
        tg = t[g].astype(LD)
        P = ray.p[None] + np.einsum("mk,kcn->mcn", tg, ray.dp)  # (M, 2, n)
        S = ray.s[None] + np.einsum("mk,kcn->mcn", tg, ray.ds)
        MP = ray.P[None] + np.einsum("mk,kcn->mcn", np.abs(t[g]), ray.DP)
        MS = ray.S[None] + np.einsum("mk,kcn->mcn", np.abs(t[g]), ray.DS)
        W, Wf = ray.W, ray.W.astype(np.float64)
        moments[g] = np.stack([np.broadcast_to(W.sum(), (M,)), (W * P[:, 0]).sum(axis=1), (W * P[:, 1]).sum(axis=1),
                               (W * S[:, 0]).sum(axis=1), (W * S[:, 1]).sum(axis=1), (W * (P * P).sum(axis=1)).sum(axis=1),
                               (W * (P * S).sum(axis=1)).sum(axis=1), (W * (S * S).sum(axis=1)).sum(axis=1)], axis=1)
        c = 2 * (K_P + n_par) + 4 + ray.n_selected + K.kMtfMaxSlices
        gamma = c * R.U64 / (1 - c * R.U64)
        moments_bound[g] = gamma * np.stack(
            [np.broadcast_to(Wf.sum(), (M,)), (Wf * MP[:, 0]).sum(axis=1), (Wf * MP[:, 1]).sum(axis=1),
             (Wf * MS[:, 0]).sum(axis=1), (Wf * MS[:, 1]).sum(axis=1), (Wf * (MP * MP).sum(axis=1)).sum(axis=1),
             (Wf * (MP * MS).sum(axis=1)).sum(axis=1), (Wf * (MS * MS).sum(axis=1)).sum(axis=1)], axis=1)
        moved[g] = (P, S, MP, MS, W, Wf)
    best, best_bound = best_focus(moments, moments_bound)
    if focus_shift is not None:
        shift = np.asarray(focus_shift, dtype=np.float64).astype(LD)
    else:
        shift = best if compensate else np.where(np.isnan(best), np.nan, 0).astype(LD)
    for g in range(n_groups):
        if moved[g] is None:
            continue
        P, S, MP, MS, W, Wf = moved[g]
        total = W.sum()
        for m in range(M):
            dm = shift[g, m]
            X = P[m] + dm * S[m]
            MX = MP[m] + abs(float(dm)) * MS[m]
            for f, delta in enumerate(planes):
                x1, x2 = X[0] + LD(delta) * S[m, 0], X[1] + LD(delta) * S[m, 1]
                for lo, hi in R._chunks(A * N, len(W) * 4):
                    cs, sn = R.phasor(KC[lo:hi] * x1[None, :] + KS[lo:hi] * x2[None, :])
                    re[g, m, f].reshape(-1)[lo:hi] = (W * cs).sum(axis=1) / total
                    im[g, m, f].reshape(-1)[lo:hi] = -(W * sn).sum(axis=1) / total
                    T = aKC[lo:hi] * MX[0] + aKS[lo:hi] * MX[1] + abs(delta) * (aKC[lo:hi] * MS[m, 0] + aKS[lo:hi] * MS[m, 1])
                    e_ray = R.EPS_TRIG + (2 * math.pi * R.F32_TURN) ** 2 / 2 + 2 * math.pi * k_t(n_par) * R.U64 * T
                    otf_bound[g, m, f].reshape(-1)[lo:hi] = (Wf * e_ray).sum(axis=1) / float(total)
    return SimpleNamespace(re=re, im=im, otf=re.astype(np.float64) + 1j * im.astype(np.float64), otf_bound=otf_bound,
                           moments=moments, moments_bound=moments_bound, best_focus=best, best_focus_bound=best_bound,
                           focus_shift=shift, **vars(rec))


def about_centroid(ref, frequencies, azimuths, focus):
    """``reference="centroid"`` of the reference: OTF exp(+2 pi i k.c_m(delta_f + delta_m)), c_m from the reference's own
    moments: complex128 (G, M, F, A, N)."""
    kc, ks = (x.astype(LD) for x in R.frequency_table(frequencies, azimuths))
    m = ref.moments
    mp, ms = m[..., 1:3] / m[..., 0, None], m[..., 3:5] / m[..., 0, None]
    planes = np.asarray(focus, dtype=np.float64).astype(LD)[None, None, :] + ref.focus_shift[:, :, None]
    c = mp[:, :, None, :] + planes[..., None] * ms[:, :, None, :]  # (G, M, F, 2)
    cs, sn = R.phasor(c[..., 0, None, None] * kc + c[..., 1, None, None] * ks)
    return ((ref.re * cs - ref.im * sn).astype(np.float64) + 1j * (ref.re * sn + ref.im * cs).astype(np.float64))


def sample_statistics(ref_rays, trials_g, shift_g, focus):
    """Per trial and plane the weighted centroid (M, F, 2) and RMS radius (M, F) of the moved points themselves, in
    longdouble: X = P + (delta_f + delta_m) S of one group's staged rays."""
    tg = np.asarray(trials_g, dtype=np.float64).astype(LD)
    P = ref_rays.p[None] + np.einsum("mk,kcn->mcn", tg, ref_rays.dp)
    S = ref_rays.s[None] + np.einsum("mk,kcn->mcn", tg, ref_rays.ds)
    W = ref_rays.W
    planes = np.asarray(focus, dtype=np.float64).astype(LD)[None, :] + np.asarray(shift_g, dtype=np.float64).astype(LD)[:, None]
    X = P[:, None] + planes[:, :, None, None] * S[:, None]  # (M, F, 2, n)
    c = (W * X).sum(axis=-1) / W.sum()
    r2 = (W * ((X - c[..., None]) ** 2).sum(axis=2)).sum(axis=-1) / W.sum()
    return c, np.sqrt(r2)


def deviation(got, re, im):
    return G.deviation(got, re, im)


# ---- the inputs of the tests (CPU and GPU) ----------------------------------------------------------------------------------
tolerance_case = G.gradient_case


def reference_of(case, trials, frequencies, azimuths=(0.0, 90.0), focus=(0.0,), centre=None, jacobian=None, slopes=None,
                 compensate=False, focus_shift=None):
    frame = case.frame
    return tolerance_reference(frame[case.rows, 9:12], frame[case.rows, 12:15], frame[case.rows, 1], case.group,
                               case.n_groups, case.jacobian if jacobian is None else jacobian,
                               case.slopes if slopes is None else slopes, trials, frequencies, azimuths, focus,
                               centre=centre, compensate=compensate, focus_shift=focus_shift)


def staged_of(case, centre=None):
    frame = case.frame
    return staged(frame[case.rows, 9:12], frame[case.rows, 12:15], frame[case.rows, 1], case.group, case.n_groups,
                  case.jacobian, case.slopes, None, centre)


def random_trials(n_trials, n_parameters, scale=2e-3, seed=5):
    """(M, K) trials of about ``scale``: with gradient_case's dQ of order 0.5 a landing point moves by about 1e-3, the
    spot's own size (mtf_case's spread 2e-3)."""
    return np.random.default_rng(seed).normal(0.0, scale, (n_trials, n_parameters))


# ray counts about the LDS tile (kMtftRays = 64) and the slice (kMtfMinSlice = 2048)
SIZES = (1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 3 * 2048 + 1)
FILLER = 2 * 2048 + 100
# trials about a wave (64: a wave whose trials all lie past M skips the work) and the tile (kMtftTile = 256)
TRIAL_COUNTS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 258, 513)
# parameters at every step of the instantiation (4, 8, 12, 16)
PARAMETER_COUNTS = (1, 3, 4, 5, 8, 9, 12, 13, 16)
# planes x azimuths x frequencies about the chunk of kMtftOut = 8 outputs
OUTPUT_COUNTS = ((1, 1, 1), (1, 1, 7), (1, 2, 4), (1, 1, 9), (3, 2, 5))

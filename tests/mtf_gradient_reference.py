"""An extended-precision reference of the MTF sensitivities (d(OTF)/d(parameter) through focus: the definitions of
include/prt.h under prt_frame_mtf_gradient), the error budget k_mtfg_stage and k_mtfg_sum are held to, Python copies of
the new partition rules and the inputs the tests run on.  It builds on tests/diffraction_reference.py (the phasor, EPS_TRIG,
K_OTF, the MTF's kept rule and its case builders) and changes nothing there.

What counts as an input: the frame's rows, ``jacobian`` and ``slopes`` (exact, whatever pass made them), the (kc, ks) table
as the library's host code forms it, and the centre C_g the device used (its own centroid is held to ``centroid``'s bound
apart from the sums).

The budget, per output and parameter (``gradient_bound``), u = 2^-53:

    |dOTF~ - dOTF| <= 2 pi [ mean_w(|g_r| e_r) + K_G u mean_w(G_r) ]

  g_r = k.dx_r = kc dp1 + ks dp2 + delta (kc ds1 + ks ds2) is the ray's term and e_r = EPS_TRIG + (2 pi 2^-25)^2 / 2
  + 2 pi K_OTF u T_r the budget of its phasor, exactly the OTF's (diffraction_reference: the phase path is k_mtf_sum's; the
  first-order correction is folded into the phasor once, (c - theta sn, sn + theta c) = (c + i sn)(1 + i theta), which
  leaves the same theta^2 / 2).  The second term is what the roundings of g_r itself cost; G_r is the sum of the
  magnitudes of the terms that enter g_r,
    G_r = |kc| DP1 + |ks| DP2 + |delta| (|kc| DS1 + |ks| DS2),  with A(x, e) = sum_c |x_c e_c|, S1 as for the OTF,
    kappa = A(u, a) / |u.a| >= 1,
    DS1 = (A(duh, e1) + S1 A(duh, a)) kappa / |uh.a| >= |ds1|,
    DP1 = A(dQ, e1) + S1 A(dQ, a) + DS1 A(d, a) >= |dp1|.
  K_G = 29 counts roundings to first order, each relative to the magnitude it acts on (k_mtfg_stage is compiled without
  contraction, so every product and sum rounds once):
    uh.a = (u.a) / |u|: the dot product 3 A(u, a), |u| = sqrt(u.u) 3 / 2 + 1 (under 3), the division 1: (3 kappa + 4) of
      |uh.a|, at most 7 kappa;
    s1 within 4 S1 (diffraction_reference);  duh.e1 3 A(duh, e1);  s1 (duh.a): 4 + 3 + 1 = 8 S1 A(duh, a);  the
      subtraction 1: the numerator of ds1 is within 9 (A(duh, e1) + S1 A(duh, a)); divided by uh.a (7 kappa, and 1 for the
      division): ds1 within 17 DS1;
    dQ.e1 3 A(dQ, e1);  s1 (dQ.a) 8 S1 A(dQ, a);  d = Q - C 1, d.a 4 A(d, a), ds1 (d.a) 17 + 4 + 1 = 22 DS1 A(d, a);  the
      two subtractions 2: dp1 within 24 DP1;
    the chain fma(kc, dp1, fma(ks, dp2, fma(kc delta, ds1, (ks delta) ds2))), as for the OTF: one rounding for each of
      kc delta and ks delta, one for the innermost product and one per fma: the dp terms carry 24 + 2 = 26, the ds terms
      17 + 1 + 1 + 3 = 22.  26;
    the phasor's last steps, relative to |g_r| <= G_r: c' = fma(-theta, sn, c) 1, w c' 1: 2;  and 1 more for the terms
      of second order.  29.
  The focus derivative has g_r = fma(kc, s1, ks s2): 4 + 2 roundings of |kc| S1 + |ks| S2, well inside the same K_G with
  DP = (S1, S2) and DS = 0.
  What the budget leaves to EPS_TRIG's margin, as the OTF's does: the fp64 accumulation of the sums (at most
  rays-per-slice times u of sum w |g|) and the normalisation.
``otf`` keeps ``otf_bound``; dC_k = sum w dQ_k / sum w keeps the form of ``centroid``'s bound with the new chunk.
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

import diffraction_reference as R

LD = R.LD
K_G = 29
MAX_PARAMETERS = 16


def kernel_constants():
    """The static const ints of prt_mtf_gradient.hpp (kMtfgBlock, kMtfgTile, ...)."""
    found = {}
    text = open(os.path.join(R.ROOT, "pyrayt_amd", "csrc", "prt_mtf_gradient.hpp")).read()
    for key, value in re.findall(r"static const (?:int|size_t) (k\w+) = ([^;]+);", text):
        value = re.sub(r"(\d+)u\b", r"\1", value)
        try:
            found[key] = int(eval(value, {"__builtins__": {}}, dict(found)))
        except (NameError, SyntaxError, TypeError):
            pass  # (not a plain constant)
    return SimpleNamespace(**found)


K = kernel_constants()
QUANTITIES = MAX_PARAMETERS + 2  # (kMtfgQuantities: the slab is sized for 16 parameters whatever K is)
# Python copies of lines of prt_frame_mtf_gradient and of mtf_slices and mtf_plan (prt_mtf.hpp) as it calls them, held to
# the headers' text by tests/test_host_mtf_gradient.py
HOST_RULES = {
    "prt_mtf_gradient.hpp": (
        "static const int kMtfgQuantities = MTFG_MAX_PARAMETERS + 2;",
        "enum { MTFG_MAX_PARAMETERS = 16, MTFG_RECORD = 7 };",
        "static_assert(kMtfgMinSlice == kMtfMinSlice && kMtfgMaxSlices == kMtfMaxSlices && kMtfgSlabBytes == kMtfSlabBytes,",
        'int rc = mtf_plan("mtf_gradient", frequencies, n_frequencies, azimuths_deg, n_azimuths, focus, n_focus, axes, n_groups,',
        "kMtfgQuantities * 16, kMtfgOut, kMtfgBlock, plan);",
        "const MtfgStaging staging(group_first, n_groups, K, plan.max_slices, workspace);",
        "h_slice[g + 1] = h_slice[g] + mtf_slices(count, max_slices);",
        "h_chunk[g + 1] = h_chunk[g] + (count + kMtfgChunk - 1) / kMtfgChunk;",
        "const int whole = K / kMtfgParams, rest = K - whole * kMtfgParams;",
        "if (rest > 4) sum(std::integral_constant<int, 8>(), 1, whole * kMtfgParams);",
        "else if (rest > 2) sum(std::integral_constant<int, 4>(), 1, whole * kMtfgParams);",
        "else if (rest == 2) sum(std::integral_constant<int, 2>(), 1, whole * kMtfgParams);",
        "else if (rest == 1) sum(std::integral_constant<int, 1>(), 1, whole * kMtfgParams);",
        "for (int64_t base = lo; base < hi; base += kMtfgTile) {"),
    "prt_mtf.hpp": (
        "const int64_t s = (count + kMtfMinSlice - 1) / kMtfMinSlice;",
        "return s < 1 ? 1 : (s > max_slices ? max_slices : s);",
        "const size_t cells = (size_t)n_groups * n_out * cell_bytes;",
        "p.max_slices = std::max<int64_t>(1, std::min<int64_t>(kMtfMaxSlices, (int64_t)(kMtfSlabBytes / cells)));",
        "const int lanes = n_out <= out * block / 4 ? 4 : (n_out <= out * block / 2 ? 2 : 1);",
        "const int64_t tile = (int64_t)out * (block / lanes), tiles = (n_out + tile - 1) / tile;"),
}


def slices(count, n_groups, n_out):
    """The ray slices of a group of ``count`` selected rows: they follow nothing but count, n_groups and n_out."""
    cap = max(1, min(K.kMtfgMaxSlices, K.kMtfgSlabBytes // (n_groups * n_out * QUANTITIES * 16)))
    return min(max(-(-count // K.kMtfgMinSlice), 1), cap)


def lanes(n_out):
    return 4 if n_out <= K.kMtfgOut * K.kMtfgBlock // 4 else (2 if n_out <= K.kMtfgOut * K.kMtfgBlock // 2 else 1)


def tile(n_out):
    """Outputs of a k_mtfg_sum workgroup."""
    return K.kMtfgOut * (K.kMtfgBlock // lanes(n_out))


def parameter_chunks(n_parameters):
    """The k_mtfg_sum launches of a call: (instantiation P, chunks of it, first parameter)."""
    whole, rest = divmod(n_parameters, K.kMtfgParams)
    out = [(K.kMtfgParams, whole, 0)] if whole else []
    if rest:
        out.append((8 if rest > 4 else 4 if rest > 2 else rest, 1, whole * K.kMtfgParams))
    return out


# ---- the reference --------------------------------------------------------------------------------------------------------
def selection(frame, surface, rays_per_source, n_groups):
    """The rows a sensitivity pass selects at ``surface``, ordered by (group, generation, id): their row numbers and
    groups."""
    ids, generation = frame[:, 4], frame[:, 0]
    group = np.floor(ids / rays_per_source).astype(np.int64) if rays_per_source else np.zeros(len(frame), dtype=np.int64)
    picked = np.flatnonzero((frame[:, 5] == surface) & (group >= 0) & (group < n_groups))
    order = np.lexsort((ids[picked], generation[picked], group[picked]))
    picked = picked[order]
    return picked, group[picked]


def _magnitude(x, e):
    return (np.abs(x) * np.abs(e)).sum(axis=1)


def gradient_reference(q, u, w, group, n_groups, jacobian, slopes, frequencies, azimuths=(0.0, 90.0), focus=(0.0,),
                       axes=None, centre=None):
    """The definitions of include/prt.h from the selected rows in their order (q, u (n, 3), w, group) and jacobian, slopes
    (K, 3, n): a namespace of re, im (G, F, A, N) longdouble (the OTF) and otf_bound; dre, dim (G, K + 1, F, A, N)
    longdouble (index K the focus derivative) and dbound; dcentroid (G, K, 3) and dcentroid_bound; centre (the one used),
    centroid, centre_bound, sum_weights, n_rays, n_missed, n_unfollowed."""
    axes = R.default_axes() if axes is None else np.asarray(axes, dtype=np.float64)
    q, u, w = (np.asarray(x, dtype=np.float64) for x in (q, u, w))
    jacobian, slopes = np.asarray(jacobian, dtype=np.float64), np.asarray(slopes, dtype=np.float64)
    n_par = len(jacobian)
    passes = R.mtf_kept(q, u, w, axes)
    followed = np.all(np.isfinite(jacobian), axis=(0, 1)) & np.all(np.isfinite(slopes), axis=(0, 1))
    a, e1, e2 = (axes[k:k + 3].astype(LD) for k in (0, 3, 6))
    kc, ks = R.frequency_table(frequencies, azimuths)
    planes = np.asarray(focus, dtype=np.float64)
    F, (A, N) = len(planes), kc.shape
    G = n_groups
    nan = lambda *shape, dtype=LD: np.full(shape, np.nan, dtype=dtype)  # noqa: E731
    re, im, otf_bound = nan(G, F, A, N), nan(G, F, A, N), nan(G, F, A, N, dtype=float)
    dre, dim, dbound = nan(G, n_par + 1, F, A, N), nan(G, n_par + 1, F, A, N), nan(G, n_par + 1, F, A, N, dtype=float)
    dcentroid, dcentroid_bound = nan(G, n_par, 3), nan(G, n_par, 3, dtype=float)
    centres, centroids, centre_bound, sums = nan(G, 3), nan(G, 3), nan(G, 3, dtype=float), nan(G)
    used, missed, unfollowed = (np.zeros(G, dtype=np.int64) for _ in range(3))
    KC, KS = kc.astype(LD).reshape(-1, 1), ks.astype(LD).reshape(-1, 1)
    aKC, aKS = np.abs(kc).reshape(-1, 1), np.abs(ks).reshape(-1, 1)
    for g in range(G):
        mine = group == g
        m = mine & passes & followed
        used[g], missed[g], unfollowed[g] = int(m.sum()), int((mine & ~passes).sum()), int((mine & passes & ~followed).sum())
        if not used[g]:
            continue
        Q, Uv, W = q[m].astype(LD), u[m].astype(LD), w[m].astype(LD)
        own, centre_bound[g] = R.centroid(q[m], w[m])
        centroids[g] = own
        c = own if centre is None else np.asarray(centre[g], dtype=np.float64).astype(LD)
        centres[g] = c
        total = W.sum()
        sums[g] = total
        if not total > 0:
            continue
        d = Q - c
        norm = np.sqrt((Uv * Uv).sum(axis=1))
        ua = (Uv @ a) / norm  # (of the unit direction)
        s1, s2 = (Uv @ e1) / (Uv @ a), (Uv @ e2) / (Uv @ a)
        da = d @ a
        p1, p2 = d @ e1 - s1 * da, d @ e2 - s2 * da
        S1, S2 = ((_magnitude(Uv, e) + np.abs(s) * _magnitude(Uv, a)) / np.abs(Uv @ a) for e, s in ((e1, s1), (e2, s2)))
        P1, P2 = _magnitude(d, e1) + S1 * _magnitude(d, a), _magnitude(d, e2) + S2 * _magnitude(d, a)
        kappa = _magnitude(Uv, a) / np.abs(Uv @ a)
        terms = []  # per parameter (dp1, dp2, ds1, ds2) and their magnitudes (DP1, DP2, DS1, DS2); the focus last
        depth = K.kMtfgChunk // K.kMtfgBlock + int(math.log2(K.kMtfgBlock)) + -(-int(mine.sum()) // K.kMtfgChunk)
        for k in range(n_par):
            dQ, dU = jacobian[k][:, m].T.astype(LD), slopes[k][:, m].T.astype(LD)
            dua, dqa = dU @ a, dQ @ a
            ds1, ds2 = (dU @ e1 - s1 * dua) / ua, (dU @ e2 - s2 * dua) / ua
            dp1, dp2 = dQ @ e1 - s1 * dqa - ds1 * da, dQ @ e2 - s2 * dqa - ds2 * da
            DS1, DS2 = ((_magnitude(dU, e) + S * _magnitude(dU, a)) * kappa / np.abs(ua) for e, S in ((e1, S1), (e2, S2)))
            DP1 = _magnitude(dQ, e1) + S1 * _magnitude(dQ, a) + DS1 * _magnitude(d, a)
            DP2 = _magnitude(dQ, e2) + S2 * _magnitude(dQ, a) + DS2 * _magnitude(d, a)
            terms.append(((dp1, dp2, ds1, ds2), tuple(x.astype(np.float64) for x in (DP1, DP2, DS1, DS2))))
            dcentroid[g, k] = (W[:, None] * dQ).sum(axis=0) / total
            dcentroid_bound[g, k] = (2 * (depth + 2) * R.U64 * (W[:, None] * np.abs(dQ)).sum(axis=0) / total).astype(float)
        zero = np.zeros(len(W))
        terms.append(((s1, s2, zero.astype(LD), zero.astype(LD)),
                      (S1.astype(np.float64), S2.astype(np.float64), zero, zero)))
        Wf = W.astype(np.float64)
        S1f, S2f, P1f, P2f = (x.astype(np.float64) for x in (S1, S2, P1, P2))
        for f, delta in enumerate(planes):
            x1, x2 = p1 + LD(delta) * s1, p2 + LD(delta) * s2
            for lo, hi in R._chunks(A * N, len(W) * 4):
                cs, sn = R.phasor(KC[lo:hi] * x1[None, :] + KS[lo:hi] * x2[None, :])
                re[g, f].reshape(-1)[lo:hi] = (W * cs).sum(axis=1) / total
                im[g, f].reshape(-1)[lo:hi] = -(W * sn).sum(axis=1) / total
                T = aKC[lo:hi] * P1f + aKS[lo:hi] * P2f + abs(delta) * (aKC[lo:hi] * S1f + aKS[lo:hi] * S2f)
                otf_bound[g, f].reshape(-1)[lo:hi] = R.otf_bound((Wf * T).sum(axis=1) / float(total))
                e_ray = R.EPS_TRIG + (2 * math.pi * R.F32_TURN) ** 2 / 2 + 2 * math.pi * R.K_OTF * R.U64 * T
                for k, ((dp1, dp2, ds1, ds2), (DP1, DP2, DS1, DS2)) in enumerate(terms):
                    gr = KC[lo:hi] * (dp1 + LD(delta) * ds1)[None, :] + KS[lo:hi] * (dp2 + LD(delta) * ds2)[None, :]
                    dre[g, k, f].reshape(-1)[lo:hi] = -R.TWO_PI * (W * gr * sn).sum(axis=1) / total
                    dim[g, k, f].reshape(-1)[lo:hi] = -R.TWO_PI * (W * gr * cs).sum(axis=1) / total
                    Gr = aKC[lo:hi] * DP1 + aKS[lo:hi] * DP2 + abs(delta) * (aKC[lo:hi] * DS1 + aKS[lo:hi] * DS2)
                    dbound[g, k, f].reshape(-1)[lo:hi] = 2 * math.pi * (
                        (Wf * np.abs(gr.astype(np.float64)) * e_ray).sum(axis=1)
                        + K_G * R.U64 * (Wf * Gr).sum(axis=1)) / float(total)
    return SimpleNamespace(re=re, im=im, otf=re.astype(np.float64) + 1j * im.astype(np.float64), otf_bound=otf_bound,
                           dre=dre, dim=dim, dotf=dre.astype(np.float64) + 1j * dim.astype(np.float64), dbound=dbound,
                           dcentroid=dcentroid, dcentroid_bound=dcentroid_bound, centre=centres, centroid=centroids,
                           centre_bound=centre_bound, sum_weights=sums, n_rays=used, n_missed=missed,
                           n_unfollowed=unfollowed, n_parameters=n_par)


def follow_centroid(ref, frequencies, azimuths, axes=None):
    """``reference="centroid"`` of the reference: dOTF_k + 2 pi i (k.(dC_k.e1, dC_k.e2)) OTF + (dC_k.a) dOTF/ddelta, in
    longdouble parts (dre, dim) (G, K, F, A, N)."""
    axes = R.default_axes() if axes is None else np.asarray(axes, dtype=np.float64)
    a, e1, e2 = (axes[k:k + 3].astype(LD) for k in (0, 3, 6))
    kc, ks = (x.astype(LD) for x in R.frequency_table(frequencies, azimuths))
    n_par = ref.n_parameters
    dc = ref.dcentroid
    shift = (dc @ e1)[:, :, None, None] * kc + (dc @ e2)[:, :, None, None] * ks  # (G, K, A, N)
    along = (dc @ a)[:, :, None, None, None]
    two_pi_shift = R.TWO_PI * shift[:, :, None]
    dre = ref.dre[:, :n_par] - two_pi_shift * ref.im[:, None] + along * ref.dre[:, n_par][:, None]
    dim = ref.dim[:, :n_par] + two_pi_shift * ref.re[:, None] + along * ref.dim[:, n_par][:, None]
    return dre, dim


def deviation(got, re, im):
    """|got - reference| per value, the difference taken in longdouble."""
    return np.hypot(np.real(got).astype(LD) - re, np.imag(got).astype(LD) - im).astype(np.float64)


# ---- the inputs of the tests (CPU and GPU) ----------------------------------------------------------------------------------
def gradient_case(counts, n_parameters, *, filler=0, left_out=0, seed=3, unfollowed=0, **mtf_case):
    """A frame of diffraction_reference.mtf_case and, for its selected rows in the pass's order, a synthetic jacobian and
    slopes (K, 3, n): dQ of order 0.5 per unit parameter, duh of order 0.3 and tangent to the unit sphere as a real
    slope is.  ``unfollowed``: that many rows of every group get a NaN in the jacobian of parameter
    ``n_parameters // 2`` alone."""
    case = R.mtf_case(counts, filler=filler, left_out=left_out, seed=seed, **mtf_case)
    rows, group = selection(case.frame, R.SURFACE, case.rays_per_source, case.n_groups)
    rng = np.random.default_rng(1000 + seed)
    n = len(rows)
    u = case.frame[rows, 12:15]
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = u / np.linalg.norm(u, axis=1, keepdims=True)
    unit = np.where(np.isfinite(unit), unit, 0.0)
    jacobian = rng.normal(0.0, 0.5, (n_parameters, 3, n)) * (1 + np.arange(n_parameters))[:, None, None] ** 0.5
    raw = rng.normal(0.0, 0.3, (n_parameters, 3, n))
    slopes = raw - unit.T[None] * np.einsum("kcn,nc->kn", raw, unit)[:, None, :]
    spoiled = np.zeros(n, dtype=bool)
    if unfollowed:
        kept = R.mtf_kept(case.frame[rows, 9:12], u, case.frame[rows, 1], R.default_axes())
        for g in range(case.n_groups):
            mine = np.flatnonzero((group == g) & kept)
            spoiled[mine[rng.permutation(len(mine))[:unfollowed]]] = True
        jacobian[n_parameters // 2, 1, spoiled] = np.nan
    return SimpleNamespace(frame=case.frame, rows=rows, group=group, jacobian=jacobian, slopes=slopes, spoiled=spoiled,
                           rays_per_source=case.rays_per_source, n_groups=case.n_groups, n_parameters=n_parameters)


def reference_of(case, frequencies, azimuths=(0.0, 90.0), focus=(0.0,), centre=None, jacobian=None, slopes=None):
    frame = case.frame
    return gradient_reference(frame[case.rows, 9:12], frame[case.rows, 12:15], frame[case.rows, 1], case.group,
                              case.n_groups, case.jacobian if jacobian is None else jacobian,
                              case.slopes if slopes is None else slopes, frequencies, azimuths, focus, centre=centre)


# ray counts about the sum's LDS tile (kMtfgTile = 128), the MTF's sizes (the slice, kMtfgMinSlice = 2048, is the MTF's)
SIZES = (1, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 1)
FILLER = 2 * 2048 + 100
# parameters: one, about the chunk of 8 (7: one launch of 8 with a zero column; 8: one whole chunk; 9: a whole chunk and a
# launch of 1), and the most
PARAMETER_COUNTS = (1, 7, 8, 9, 16)
# planes x azimuths x frequencies about the output tile: 128 outputs (lanes = 4), 256 (lanes = 2), 512 (lanes = 1)
OUTPUT_COUNTS = ((1, 1, 127), (4, 4, 8), (1, 3, 43), (4, 4, 16), (1, 1, 257), (8, 4, 16), (3, 9, 19))

"""A numpy / longdouble restatement of the Monte Carlo tolerancing of the enclosed energy (the definitions of
include/prt.h under prt_frame_energy_tolerance), the band every ray's distance is held to, and the inputs the tests run
on.  It stands on tests/mtf_tolerance_reference.py (the staged quantities, their counted roundings, its case builders and
slice rules) and on tests/energy_reference.py (``integer_weights``, ``clear_radii``) and changes neither.

What counts as an input: the frame's rows, ``jacobian`` and ``slopes``, the trials, the held centre C_g the device used,
the focus shift delta_m it applied (held to ``best_focus_bound`` by the MTF tolerancing's own tests: the two passes give
the same bits) and, with follow_centroid, the trial's moments as the device wrote them (``moments_out``, held to
``moments_bound`` there): the centre of a plane is a float64 line on them,
    c = m_P / m_0 + delta * (m_S / m_0),   delta = focus[f] + delta_m,
quotients, product and sums each rounded on their own, which ``plane_centres`` restates and the device reproduces bit for
bit.  With c and delta given, the only thing the device rounds differently from this reference is the ray.

The band eps_r of a ray's distance (u = 2^-53).  From mtf_tolerance_reference's count the chains of a trial of K
parameters give P within (24 + K) u MP and S within (17 + K) u MS, MP = P + sum |t_k| DP_k and MS likewise the chains'
magnitudes.  The point in the plane is formed without fma, fl(P + fl(delta S)): the product and the sum round once each,
so X is within (26 + K) u MX, MX = MP + |delta| MS (the MTF tolerancing's fma(delta, S, P) rounds once: 25 + K there).
The subtraction of the centre rounds once more on |X| + |c|; with one rounding for the terms of second order
    |x~_i - x_i| <= e_i = (28 + K) u (MX_i + |c_i|)         per component i.
The shapes: a slit |x_i| adds nothing, eps = e_i; the square max(|x_1|, |x_2|) is 1-Lipschitz in each, eps = max(e_1,
e_2); the circle sqrt(fl(fl(x_1^2) + fl(x_2^2))) moves by at most |e| <= e_1 + e_2 with its arguments and rounds
relatively three times under the root (two products, one sum: 3 u of d^2, 1.5 u of d) and once on it,
eps = e_1 + e_2 + 3 u d.  The device's distance lies in [d - eps, d + eps], d this reference's longdouble distance.

Every check is then an exact integer inequality, no float tolerance:
    counts   sum q [d + eps < R]  <=  count  <=  sum q [d - eps <= R]
    radius   for the device's d*:  sum q [d + eps < d*] < T  and  sum q [d - eps <= d*] >= T,  T = clamp(ceil(phi W), 1, W)
and the tests choose their radii at gaps of the union of all trials' distances (``clear_radii``, relative gap 1e-9, a
million bands wide), so that no (trial, plane, radius) cell has a ray in its band: ``undecided`` is 0, asserted, and
the counts are compared for equality.
The integer weights: include/prt.h takes B from the group's count of SELECTED rows (a row that is left out is staged with
w = 0), so ``integer_weights`` here is energy_reference's on the kept weights padded with zeros to that count; W is its
integer sum."""
from types import SimpleNamespace

import numpy as np

import diffraction_reference as R
import energy_reference as E
import mtf_tolerance_reference as T

LD = R.LD
U = R.U64
SHAPES = E.SHAPES


def k_x(n_parameters):
    return 28 + n_parameters


def integer_weights(kept_weights, n_selected):
    """q of the kept rays: energy_reference.integer_weights over the group's selected rows, the others with w = 0."""
    w = np.asarray(kept_weights, dtype=np.float64)
    return E.integer_weights(np.concatenate([w, np.zeros(n_selected - len(w))]))[:len(w)]


def needs(total, fractions):
    """T_k = clamp(ceil(phi_k W), 1, W) in the device's float64 arithmetic."""
    return np.array([min(max(int(np.ceil(np.float64(phi) * np.float64(total))), 1), total) for phi in fractions],
                    dtype=np.uint64)


def plane_centres(moments, delta, follow_centroid):
    """(M, F, 2) float64: the line of the docstring on float64 ``moments`` (M, 8) and ``delta`` (M, F); zeros about the held
    centre."""
    m = np.asarray(moments, dtype=np.float64)
    if not follow_centroid:
        return np.zeros(delta.shape + (2,))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mp, ms = m[:, 1:3] / m[:, 0:1], m[:, 3:5] / m[:, 0:1]
        return mp[:, None, :] + delta[:, :, None] * ms[:, None, :]


def shape_distance(x, shape):
    """d of x (..., 2, n) in x's own precision."""
    if shape == "circle":
        return np.sqrt(x[..., 0, :] * x[..., 0, :] + x[..., 1, :] * x[..., 1, :])
    if shape == "square":
        return np.maximum(np.abs(x[..., 0, :]), np.abs(x[..., 1, :]))
    if shape == "slit_e2":
        return np.abs(x[..., 0, :])
    if shape == "slit_e1":
        return np.abs(x[..., 1, :])
    raise ValueError(shape)


def shape_band(e, d, shape):
    if shape == "circle":
        return e[..., 0, :] + e[..., 1, :] + 3 * U * d.astype(np.float64)
    if shape == "square":
        return np.maximum(e[..., 0, :], e[..., 1, :])
    return e[..., 0, :] if shape == "slit_e2" else e[..., 1, :]


def moments_of(P, S, W):
    """(M, 8) longdouble: sum w, sum w P (2), sum w S (2), sum w P.P, sum w P.S, sum w S.S of moved rays (M, 2, n)."""
    M = len(P)
    return np.stack([np.broadcast_to(W.sum(), (M,)), (W * P[:, 0]).sum(axis=1), (W * P[:, 1]).sum(axis=1),
                     (W * S[:, 0]).sum(axis=1), (W * S[:, 1]).sum(axis=1), (W * (P * P).sum(axis=1)).sum(axis=1),
                     (W * (P * S).sum(axis=1)).sum(axis=1), (W * (S * S).sum(axis=1)).sum(axis=1)], axis=1)


def energy_tolerance_reference(q, u, w, group, n_groups, jacobian, slopes, trials, focus=(0.0,), shape="circle",
                               follow_centroid=True, axes=None, centre=None, compensate=False, moments=None,
                               focus_shift=None):
    """Per group a namespace (None for a group without kept rays or weight) of d (M, F, n) longdouble, the distances of
    the kept rays in every trial and plane; eps (M, F, n) float64, their bands; q (n) uint64 and W (a Python int);
    moments (M, 8) longdouble, this reference's own; shift (M) and delta (M, F) float64, centres (M, F, 2) float64 as
    they were used.  ``trials``: (M, K) for every group or (G, M, K).  ``moments`` (G, M, 8) and ``focus_shift`` (G, M):
    the device's, where given; else this reference's own moments rounded to float64, and its own least-squares focus with
    ``compensate`` or 0.  Also the record (centre, sum_weights, n_rays, n_missed, n_unfollowed)."""
    rays, rec = T.staged(q, u, w, group, n_groups, jacobian, slopes, axes, centre)
    n_par = rec.n_parameters
    t = np.asarray(trials, dtype=np.float64)
    t = np.broadcast_to(t[None], (n_groups,) + t.shape) if t.ndim == 2 else t
    planes = np.asarray(focus, dtype=np.float64)
    out = []
    for g, ray in enumerate(rays):
        if ray is None:
            out.append(None)
            continue
        tg = t[g].astype(LD)
        P = ray.p[None] + np.einsum("mk,kcn->mcn", tg, ray.dp)  # (M, 2, n)
        S = ray.s[None] + np.einsum("mk,kcn->mcn", tg, ray.ds)
        MP = ray.P[None] + np.einsum("mk,kcn->mcn", np.abs(t[g]), ray.DP)
        MS = ray.S[None] + np.einsum("mk,kcn->mcn", np.abs(t[g]), ray.DS)
        own = moments_of(P, S, ray.W)
        if focus_shift is not None:
            shift = np.asarray(focus_shift[g], dtype=np.float64)
        else:
            shift = T.best_focus(own).astype(np.float64) if compensate else np.zeros(len(P))
        used = own.astype(np.float64) if moments is None else np.asarray(moments[g], dtype=np.float64)
        delta = planes[None, :] + shift[:, None]  # (M, F), the device's one rounded sum
        c = plane_centres(used, delta, follow_centroid)
        X = P[:, None] + delta.astype(LD)[:, :, None, None] * S[:, None]  # (M, F, 2, n)
        d = shape_distance(X - c.astype(LD)[..., None], shape)
        MX = MP[:, None] + np.abs(delta)[:, :, None, None] * MS[:, None]
        e = k_x(n_par) * U * (MX + np.abs(c)[..., None])
        weights = integer_weights(ray.W.astype(np.float64), ray.n_selected)
        out.append(SimpleNamespace(d=d, eps=shape_band(e, d, shape), q=weights, W=int(weights.sum(dtype=np.uint64)),
                                   moments=own, shift=shift, delta=delta, centres=c, P=P, S=S))
    return SimpleNamespace(groups=out, **vars(rec))


def _sum(mask, q):
    return np.where(mask, q, np.uint64(0)).sum(axis=-1, dtype=np.uint64)


def count_bounds(grp, radii):
    """(lower, upper) (M, F, R) uint64 of the docstring's inequality for one group's namespace."""
    radii = np.asarray(radii, dtype=np.float64).astype(LD)
    lo, hi = (grp.d + grp.eps)[..., None, :], (grp.d - grp.eps)[..., None, :]
    edge = radii[None, None, :, None]
    return _sum(lo < edge, grp.q), _sum(hi <= edge, grp.q)


def counts_in_float64(grp, radii):
    """(M, F, R) uint64: sum q [d <= R] with d rounded to float64 -- the truth where every operation is exact."""
    d = grp.d.astype(np.float64)[..., None, :]
    return _sum(d <= np.asarray(radii, dtype=np.float64)[None, None, :, None], grp.q)


def radius_conditions(grp, fractions, radius):
    """For the radii ``radius`` (M, F, N) a pass returned: (below, reached) boolean (M, F, N), the two conditions of the
    docstring; both must hold everywhere."""
    need = needs(grp.W, fractions)[None, None, :]
    star = np.asarray(radius, dtype=np.float64).astype(LD)[..., None]  # (M, F, N, 1)
    lo, hi = (grp.d + grp.eps)[..., None, :], (grp.d - grp.eps)[..., None, :]
    return _sum(lo < star, grp.q) < need, _sum(hi <= star, grp.q) >= need


def radius_in_float64(grp, fractions):
    """(M, F, N) float64: the smallest float64 distance whose cumulative integer weight reaches T."""
    d = grp.d.astype(np.float64)
    need = needs(grp.W, fractions)
    out = np.empty(d.shape[:2] + (len(need),))
    for m in range(d.shape[0]):
        for f in range(d.shape[1]):
            order = np.argsort(d[m, f], kind="stable")
            run = np.cumsum(grp.q[order], dtype=np.uint64)
            out[m, f] = d[m, f][order][np.searchsorted(run, need, side="left")]
    return out


def clear_radii(ref, count, gap=1e-9):
    """``count`` ascending radii at gaps of the union of every group's, trial's and plane's distances, no ray within
    ``gap`` (relative: about a million bands) of any of them."""
    samples = np.concatenate([grp.d.astype(np.float64).ravel() for grp in ref.groups if grp is not None])
    return E.clear_radii(samples, count, gap)


def undecided(grp, radii):
    """The share of (trial, plane, radius) cells with a ray in its band."""
    lower, upper = count_bounds(grp, radii)
    return float(np.mean(lower != upper))


# ---- the inputs of the tests (CPU and GPU) ----------------------------------------------------------------------------------
tolerance_case = T.tolerance_case
random_trials = T.random_trials


def reference_of(case, trials, focus=(0.0,), shape="circle", follow_centroid=True, centre=None, jacobian=None, slopes=None,
                 compensate=False, moments=None, focus_shift=None):
    frame = case.frame
    return energy_tolerance_reference(frame[case.rows, 9:12], frame[case.rows, 12:15], frame[case.rows, 1], case.group,
                                      case.n_groups, case.jacobian if jacobian is None else jacobian,
                                      case.slopes if slopes is None else slopes, trials, focus, shape, follow_centroid,
                                      centre=centre, compensate=compensate, moments=moments, focus_shift=focus_shift)


def lattice_case(n, n_parameters=3, seed=1):
    """A frame, jacobian, slopes and trials on a dyadic lattice, for the held centre (0, 0, 0): end points (0, y, z) with y,
    z multiples of 1/8 in [-2, 2], so that many rays share a distance and lie exactly on radii like 1, 5/4 or 2; half the
    rays along the axis (s = 0) with slope derivatives that are multiples of 1/4, the others with slopes that are multiples
    of 1/4 and no slope derivative (so ds = 0 exactly, whatever |u| is); dQ multiples of 1/4 across the axis; weights 1/4,
    1/2, 1, 3; trials multiples of 1/8.  Every product and sum of the staging, the move, the plane and the distance is then
    exact in float64 (the root of the circle is correctly rounded), and plain float64 numpy is the truth.  Returns (case,
    trials (M, K), focus)."""
    rng = np.random.default_rng(seed)
    frame = np.zeros((n, 15))
    frame[:, 1] = rng.choice([0.25, 0.5, 1.0, 3.0], n)
    frame[:, 2], frame[:, 3], frame[:, 5] = 0.55, 1.0, R.SURFACE
    frame[:, 4] = np.arange(n)
    frame[:, 10:12] = rng.integers(-16, 17, (n, 2)) / 8.0
    frame[:, 12] = 1.0
    axial = np.arange(n) % 2 == 0
    frame[~axial, 13:15] = rng.integers(-2, 3, (int((~axial).sum()), 2)) / 4.0
    jacobian = np.zeros((n_parameters, 3, n))
    jacobian[:, 1:, :] = rng.integers(-4, 5, (n_parameters, 2, n)) / 4.0
    slopes = np.zeros((n_parameters, 3, n))
    slopes[:, 1:, axial] = rng.integers(-2, 3, (n_parameters, 2, int(axial.sum()))) / 4.0
    trials = rng.integers(-4, 5, (6, n_parameters)) / 8.0
    case = SimpleNamespace(frame=frame, rows=np.arange(n), group=np.zeros(n, dtype=np.int64), jacobian=jacobian,
                           slopes=slopes, rays_per_source=None, n_groups=1, n_parameters=n_parameters)
    return case, trials, (0.0, 0.5, -0.25)


# ray counts about the LDS tile (kMtftRays = 64) and the slice (kMtfMinSlice = 2048)
SIZES = (1, 63, 64, 65, 2048, 2049, 3 * 2048 + 1)
FILLER = T.FILLER
TRIAL_COUNTS = (1, 255, 256, 257, 1025)
PARAMETER_COUNTS = (1, 4, 5, 8, 9, 12, 13, 16)
# (planes, radii) about the chunk of kEtolOut = 8 outputs, plane-major: one output; 7 and 9 in one plane; 3 planes of 3
# (a chunk that holds three planes and one that begins inside a plane); 8 exactly; 2 planes of 8
OUTPUT_COUNTS = ((1, 1), (1, 7), (1, 9), (3, 3), (2, 4), (2, 8))
FRACTION_COUNTS = (1, 4, 5, 16)

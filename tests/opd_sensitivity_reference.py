"""Wavefront sensitivities in numpy ``longdouble``: what DeviceFrame.sensitivity(wavefront=) computes, restated from the
formulas of include/prt.h and not from the kernel.  The tangents (dx, dd) are tests/design_reference.py's; what is new
here is the plane dnu read out row by row, the differentiated optical path dL, a longdouble statement of the OPD
definitions of DeviceFrame.wavefront (the cumulative optical path, the larger root s, E, the pupil point, Zernike
polynomials from their factorial formula, not the kernel's recurrence) and the sums on top of them.

A frame, a surface table and a parameter are design_reference's.  A reference sphere is a dict: ``P`` (3,), ``R``,
``pivot``, ``pupil_radius``, ``e1`` and ``e2`` (3,)."""
from math import factorial

import numpy as np

import design_reference as dref
import sensitivity_reference as sref
from sensitivity_reference import GEN, ID, INDEX, LD, OFFSET, SURFACE, TILT, X0, X1

INTENSITY = sref.INTENSITY


def optical_path(frame):
    """The cumulative optical path of every row: index * |x1 - x0| plus the value of the same ray's row one generation
    earlier (0 where there is none)."""
    wide = np.asarray(frame, dtype=float).astype(LD)
    run = wide[:, X1] - wide[:, X0]
    segment = wide[:, INDEX] * np.sqrt(np.sum(run * run, axis=1))
    total = np.zeros(len(wide), dtype=LD)
    generations = np.asarray(frame)[:, GEN].astype(int)
    before = {}
    for g in range(generations.max() + 1 if len(wide) else 0):
        here = np.flatnonzero(generations == g)
        now = {}
        for r in here:
            total[r] = before.get(frame[r, ID], LD(0)) + segment[r]
            now[frame[r, ID]] = total[r]
        before = now
    return total


def trace(frame, table, parameters):
    """design_reference.trace_tangents, and on top of it per parameter and row dnu (the derivative of the index of the
    row's segment) and dL (the derivative of the row's cumulative optical path): a dict dx, dd, dnu, dL, count, previous."""
    frame = np.asarray(frame, dtype=float)
    info = {}
    dx, dd, count = dref.trace_tangents(frame, table, parameters, info)
    wide = frame.astype(LD)
    rows, K = len(frame), len(parameters)
    previous, kind = info["previous"], info["kind"]
    o, x, d = wide[:, X0], wide[:, X1], sref._unit(wide[:, TILT])
    run = x - o
    length = np.sqrt(np.sum(run * run, axis=1))
    # the ray enters where the trace's own normal, normal_scale included, was not turned against it
    entered = np.zeros(rows, dtype=bool)
    for sid in np.unique(frame[:, SURFACE]):
        at = frame[:, SURFACE] == sid
        if int(sid) in table and sid == int(sid):
            raw, _ = sref.surface_normals(table[int(sid)], x[at], np.zeros_like(d[at]))
            with np.errstate(invalid="ignore"):
                entered[at] = ~(np.sum(raw * d[at], axis=1) > 0)
    dnu = np.zeros((K, rows), dtype=LD)
    dL = np.full((K, rows), np.nan, dtype=LD)
    generations = frame[:, GEN].astype(int)
    for g in range(generations.max() + 1 if rows else 0):
        here = np.flatnonzero(generations == g)
        p = previous[here]
        for k, par in enumerate(parameters):
            if g == 0:
                start = np.zeros((len(here), 3), dtype=LD)
                before = np.zeros(len(here), dtype=LD)
            else:
                named = np.isin(frame[p, SURFACE], list(par["index_ids"])) & entered[p]
                dnu[k, here] = np.where(kind[here] == 1, np.where(named, LD(par["rate"]), LD(0)), dnu[k, p])
                start = dx[k, p] + OFFSET * dd[k, here]
                before = dL[k, p]
            dL[k, here] = (before + dnu[k, here] * length[here]
                           + wide[here, INDEX] * np.sum(d[here] * (dx[k, here] - start), axis=1))
    return dict(dx=dx, dd=dd, dnu=dnu, dL=dL, count=count, previous=previous)


def extend(frame, rows, P, R):
    """s (the larger root of |Q - s u - P| = R, NaN for a line that misses the sphere) and E = Q - s u of ``rows``."""
    wide = np.asarray(frame, dtype=float).astype(LD)
    q, u = wide[rows][:, X1], wide[rows][:, TILT]
    d = q - np.asarray(P, dtype=LD)
    a, b = np.sum(u * u, axis=1), np.sum(d * u, axis=1)
    c = np.sum(d * d, axis=1) - LD(R) * LD(R)
    disc = b * b - a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        root = np.sqrt(np.where(disc >= 0, disc, np.nan))
        s = np.where(b >= 0, (b + root) / a, -c / (root - b))
    return s, q - s[:, None] * u


def opd_of(frame, rows, sphere, path=None):
    """The OPD about the pivot and the normalised pupil point of ``rows`` against the sphere, held where it is."""
    wide = np.asarray(frame, dtype=float).astype(LD)
    path = optical_path(frame) if path is None else path
    s, e = extend(frame, rows, sphere["P"], sphere["R"])
    opd = path[rows] - wide[rows, INDEX] * s - LD(sphere["pivot"])
    v = e - np.asarray(sphere["P"], dtype=LD)
    pupil = np.stack([v @ np.asarray(sphere["e1"], dtype=LD), v @ np.asarray(sphere["e2"], dtype=LD)], axis=1)
    return opd, pupil / LD(sphere["pupil_radius"])


def default_sphere(frame, rows, e1=(0, 1, 0), e2=(0, 0, 1), pupil_radius=None, P=None, R=None):
    """The sphere DeviceFrame.wavefront takes by default for the group ``rows``: P the mean landing point, R the distance
    from P to the mean start of the segments, the pivot the first row whose line meets it, the pupil radius the largest
    radial extent."""
    wide = np.asarray(frame, dtype=float).astype(LD)
    P = wide[rows][:, X1].mean(axis=0) if P is None else np.asarray(P, dtype=LD)
    if R is None:
        gap = wide[rows][:, X0].mean(axis=0) - P
        R = np.sqrt(np.sum(gap * gap))
    sphere = dict(P=P, R=LD(R), pivot=LD(0), pupil_radius=LD(1), e1=np.asarray(e1, dtype=LD), e2=np.asarray(e2, dtype=LD))
    opd, pupil = opd_of(frame, rows, sphere)
    meets = np.flatnonzero(np.isfinite(opd.astype(float)))
    sphere["pivot"] = opd[meets[0]] if len(meets) else LD(np.nan)
    if pupil_radius is None:
        pupil_radius = np.sqrt(np.sum(pupil[meets] ** 2, axis=1)).max() if len(meets) else LD(np.nan)
    sphere["pupil_radius"] = LD(pupil_radius)
    return sphere


def wavefront(frame, rows, tangents, sphere):
    """Per parameter and selected row: dfield, dopd (K, n), dpupil (K, 2, n) and dE (K, n, 3); per row s, opd and pupil.
    NaN for a ray that misses the sphere or was not followed."""
    wide = np.asarray(frame, dtype=float).astype(LD)
    rows = np.asarray(rows)
    n, u = wide[rows, INDEX], sref._unit(wide[rows][:, TILT])
    opd, pupil = opd_of(frame, rows, sphere)
    s, e = extend(frame, rows, sphere["P"], sphere["R"])
    ep = e - np.asarray(sphere["P"], dtype=LD)
    dx, dd = tangents["dx"][:, rows], tangents["dd"][:, rows]
    dnu, dL = tangents["dnu"][:, rows], tangents["dL"][:, rows]
    with np.errstate(invalid="ignore", divide="ignore"):
        dfield = dL - s * dnu - n * np.sum(u * dx, axis=2)
        y = dx - s[None, :, None] * dd
        ds = np.sum(ep * y, axis=2) / np.sum(ep * u, axis=1)
        dE = y - ds[:, :, None] * u
        dopd = dfield + n * np.sum(u * dE, axis=2)
        dpupil = np.stack([dE @ np.asarray(sphere["e1"], dtype=LD), dE @ np.asarray(sphere["e2"], dtype=LD)],
                          axis=1) / LD(sphere["pupil_radius"])
    followed = np.all(np.isfinite(dx.astype(float)), axis=(0, 2))
    met = np.isfinite(opd.astype(float))
    lost = ~(followed & met)
    for value in (dfield, dopd):
        value[:, lost] = np.nan
    dpupil[:, :, lost] = np.nan
    dE[:, lost] = np.nan
    opd = np.where(lost, np.nan, opd)
    pupil = np.where(lost[:, None], np.nan, pupil)
    return dict(dfield=dfield, dopd=dopd, dpupil=dpupil, dE=dE, s=s, opd=opd, pupil=pupil, followed=followed, met=met,
                n=n, u=wide[rows][:, TILT])


def noll(j):
    n, k = 0, j - 1
    while k > n:
        n += 1
        k -= n
    m = n % 2 + 2 * ((k + (n + 1) % 2) // 2)
    return n, (-m if j % 2 else m)


def zernike(terms, x, y):
    """Z_1..Z_terms (Noll, RMS-normalised) at the pupil points (x, y): (terms, n) longdouble, from the factorial formula."""
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    rho, theta = np.sqrt(x * x + y * y), np.arctan2(y, x)
    out = []
    for j in range(1, terms + 1):
        n, m = noll(j)
        am = abs(m)
        radial = sum(LD((-1) ** k * factorial(n - k)) / LD(factorial(k) * factorial((n + am) // 2 - k)
                                                            * factorial((n - am) // 2 - k)) * rho ** (n - 2 * k)
                     for k in range((n - am) // 2 + 1))
        norm = np.sqrt(LD(n + 1)) if m == 0 else np.sqrt(LD(2 * (n + 1)))
        angular = LD(1) if m == 0 else (np.cos(am * theta) if m > 0 else np.sin(am * theta))
        out.append(norm * radial * angular)
    return np.array(out, dtype=LD)


def sums(wave, w, terms):
    """The wavefront sums of include/prt.h over the rows that are finite throughout, as a dict."""
    w = np.asarray(w, dtype=LD)
    keep = np.isfinite(w.astype(float)) & np.isfinite(wave["opd"].astype(float))
    keep &= np.all(np.isfinite(wave["dfield"].astype(float)), axis=0) & np.all(np.isfinite(wave["dopd"].astype(float)), axis=0)
    missed = wave["followed"] & ~wave["met"]
    w, opd, pupil = w[keep], wave["opd"][keep], wave["pupil"][keep]
    dfield, dopd = wave["dfield"][:, keep], wave["dopd"][:, keep]
    z = zernike(terms, pupil[:, 0], pupil[:, 1])
    nu = (wave["n"][:, None] * wave["u"])[keep]
    return {
        "count": int(keep.sum()), "missed": int(missed.sum()), "w": w.sum(), "w_opd": (w * opd).sum(),
        "w_opd2": (w * opd * opd).sum(), "z_dfield": np.einsum("jn,n,kn->kj", z, w, dfield),
        "z_nu": np.einsum("jn,n,nc->cj", z, w, nu), "w_dopd": dopd @ w, "w_opd_dopd": dopd @ (w * opd),
        "w_dfield": dfield @ w, "w_opd_dfield": dfield @ (w * opd), "moments": np.einsum("n,jn,kn->jk", w, dfield, dfield),
        "zwz": np.einsum("in,n,jn->ij", z, w, z), "z_opd": z @ (w * opd),
    }


def unpack(sums_row, K, J):
    """One group's device sums as the dict ``sums`` returns (without zwz and z_opd, which the Wavefront holds)."""
    s = np.asarray(sums_row, dtype=LD)
    at = 5 + J * (K + 3)
    z = s[5:at].reshape(K + 3, J)
    lower = np.zeros((K, K), dtype=LD)
    lower[np.tril_indices(K)] = s[at + 4 * K:]
    return {"count": int(s[0]), "missed": int(s[1]), "w": s[2], "w_opd": s[3], "w_opd2": s[4], "z_dfield": z[:K],
            "z_nu": z[K:], "w_dopd": s[at:at + K], "w_opd_dopd": s[at + K:at + 2 * K], "w_dfield": s[at + 2 * K:at + 3 * K],
            "w_opd_dfield": s[at + 3 * K:at + 4 * K], "moments": lower + np.tril(lower, -1).T}


def fit(zwz, rhs):
    """The least-squares coefficients of the normal equations, minimum norm, in float64 as solve_normal_equations has it."""
    from pyrayt_amd.frame import RANK_RCOND

    return np.linalg.lstsq(np.asarray(zwz, dtype=float), np.asarray(rhs, dtype=float), rcond=RANK_RCOND)[0]


def statistics(total):
    """From a dict of ``sums``: the variance of the piston-removed OPD, its gradient (K,) and that of the RMS."""
    w = total["w"]
    mean = total["w_opd"] / w
    variance = total["w_opd2"] / w - mean * mean
    gradient = 2 * (total["w_opd_dopd"] / w - mean * total["w_dopd"] / w)
    return dict(variance=variance, variance_gradient=gradient, rms_gradient=gradient / (2 * np.sqrt(variance)))

"""Differential ray tracing with shape and index parameters in numpy ``longdouble``: what DeviceFrame.sensitivity computes
for a mix of Motion, Deformation and IndexChange, restated from the formulas of include/prt.h and not from the kernel.
The normals and Hessians of the five primitives are tests/sensitivity_reference.py's; what is new here is the general
velocity u = v + w x (x - c) + S (x - c), the normal of a material point of a deformed surface, the plane of state dnu
(d index of the ray's segment / d parameter) and the dmu terms of Snell's law.

A frame and a surface table are sensitivity_reference's.  A parameter is a dict: ``v``, ``w``, ``c`` (3,), ``S`` (3, 3),
``ids`` (the surfaces it moves), ``rate`` and ``index_ids`` (the surfaces behind which the index grows by ``rate``)."""
import numpy as np

import sensitivity_reference as ref
from sensitivity_reference import EPS_DIR, GEN, ID, INDEX, LD, OFFSET, SURFACE, TILT, X0, X1, group_sums, table_of, unpack  # noqa: F401


def parameter(p):
    """The dict of a pyrayt_amd Motion, Deformation or IndexChange."""
    if hasattr(p, "rate"):
        return dict(v=np.zeros(3), w=np.zeros(3), c=np.zeros(3), S=np.zeros((3, 3)), ids=set(), rate=float(p.rate),
                    index_ids=set(p.surface_ids))
    return dict(v=np.asarray(p.translate, dtype=float), w=np.asarray(p.rotate, dtype=float),
                c=np.asarray(p.pivot, dtype=float), S=np.asarray(getattr(p, "linear", np.zeros((3, 3))), dtype=float),
                ids=set(p.surface_ids), rate=0.0, index_ids=set())


def velocity(par, moved, x):
    """u (n, 3) at the points x of surfaces that parameter ``par`` moves (``moved`` (n,) bool), 0 elsewhere."""
    r = x - np.asarray(par["c"], dtype=LD)
    u = np.asarray(par["v"], dtype=LD) + np.cross(np.asarray(par["w"], dtype=LD), r) + r @ np.asarray(par["S"], dtype=LD).T
    return np.where(moved[:, None], u, LD(0))


def moved_normal(par, moved, n):
    """dn of a material point of a moved surface: w x n - (I - n n^T) S^T n."""
    q = n @ np.asarray(par["S"], dtype=LD)  # (S^T n, row by row)
    dn = np.cross(np.asarray(par["w"], dtype=LD), n) - (q - n * np.sum(n * q, axis=1)[:, None])
    return np.where(moved[:, None], dn, LD(0))


def trace_tangents(frame, table, parameters, info=None):
    """dx (K, R, 3): d(landing point)/d(parameter) of every row, NaN where the ray cannot be followed; dd (K, R, 3): the
    derivative of the row's direction; a dict of the counters.  ``info``, if a dict, gets the per-row geometry the error
    budget of tests/test_gpu_design_sensitivity.py needs."""
    frame = np.asarray(frame, dtype=float)
    wide = frame.astype(LD)
    rows, K = len(frame), len(parameters)
    dx = np.full((K, rows, 3), np.nan, dtype=LD)
    dd = np.full((K, rows, 3), np.nan, dtype=LD)
    dnu = np.zeros((K, rows), dtype=LD)
    alive = np.zeros(rows, dtype=bool)
    entered = np.zeros(rows, dtype=bool)  # (the trace's normal at the row's landing was not turned: the ray enters)
    count = {"n_unknown": 0, "n_invalid": 0, "n_unfit": 0, "n_reflections": 0}
    generations = frame[:, GEN].astype(int)
    previous = None
    normals = np.full((rows, 3), np.nan, dtype=LD)
    curvature = np.zeros((rows, 3, 3), dtype=LD)
    if info is not None:
        info.update(previous=np.full(rows, -1), nd=np.full(rows, np.nan), t=np.zeros(rows), kappa=np.zeros(rows),
                    conditioning=np.ones(rows), kind=np.zeros(rows, dtype=int), mu=np.ones(rows), ct=np.ones(rows),
                    gamma=np.zeros(rows), nt=np.ones(rows), dmu=np.zeros(rows))
    for g in range(generations.max() + 1 if rows else 0):
        here = np.flatnonzero(generations == g)
        ids = frame[here, ID]
        o, x, d = wide[here, X0], wide[here, X1], ref._unit(wide[here, TILT])
        t = np.sum((x - o) * d, axis=1)
        n = np.full((len(here), 3), np.nan, dtype=LD)
        w_op = np.zeros((len(here), 3, 3), dtype=LD)
        known = np.zeros(len(here), dtype=bool)
        enters = np.zeros(len(here), dtype=bool)
        for sid in np.unique(frame[here, SURFACE]):
            at = frame[here, SURFACE] == sid
            if int(sid) in table and sid == int(sid):
                known[at] = True
                cond = np.ones(int(at.sum()))
                n[at], w_op[at] = ref.surface_normals(table[int(sid)], x[at], d[at], cond)
                raw, _ = ref.surface_normals(table[int(sid)], x[at], np.zeros_like(d[at]))  # (d = 0: never turned)
                with np.errstate(invalid="ignore"):
                    enters[at] = ~(np.sum(raw * d[at], axis=1) > 0)
                if info is not None:
                    info["conditioning"][here[at]] = cond
        finite = np.all(np.isfinite(frame[here][:, 6:15]), axis=1) & np.all(np.isfinite(d), axis=1)
        nd = np.sum(n * d, axis=1)
        with np.errstate(invalid="ignore"):
            bad_landing = ~finite | (known & ~(nd < 0))
        unknown = finite & ~known
        start_o = np.zeros((K, len(here), 3), dtype=LD)
        start_d = np.zeros((K, len(here), 3), dtype=LD)
        new_nu = np.zeros((K, len(here)), dtype=LD)
        ok = np.ones(len(here), dtype=bool)
        unfit = np.zeros(len(here), dtype=bool)
        bad_interface = np.zeros(len(here), dtype=bool)
        if g > 0:
            sorted_ids, sorted_rows = previous
            where = np.minimum(np.searchsorted(sorted_ids, ids), len(sorted_ids) - 1)
            assert np.array_equal(sorted_ids[where], ids), "a ray has a row in a generation and none in the one before"
            p = sorted_rows[where]
            ok = alive[p].copy()
            dp, np_, wp, xp = ref._unit(wide[p, TILT]), normals[p], curvature[p], wide[p, X1]
            ni, nt = wide[p, INDEX], wide[here, INDEX]
            with np.errstate(invalid="ignore", divide="ignore"):
                good_index = (ni > 0) & np.isfinite(ni) & (nt > 0) & np.isfinite(nt)
                deviation = np.sum((dp - d) ** 2, axis=1)
                refract = good_index & (ni != nt)
                reflect = good_index & (ni == nt) & (deviation > EPS_DIR)
                mu = ni / nt
                ci = -np.sum(np_ * dp, axis=1)
                radicand = 1 - mu * mu * (1 - ci * ci)
                ct = np.sqrt(np.where(radicand > 0, radicand, np.nan))
                gamma = mu * ci - ct
                want = np.where(refract[:, None], mu[:, None] * dp + gamma[:, None] * np_,
                                np.where(reflect[:, None], dp + 2 * ci[:, None] * np_, d))
                fits = np.sum((want - d) ** 2, axis=1) <= EPS_DIR
            bad_interface = ~good_index
            if info is not None:
                info["previous"][here] = p
                info["kind"][here] = np.where(refract, 1, np.where(reflect, 2, 0))
                info["mu"][here], info["ct"][here], info["gamma"][here] = mu.astype(float), ct.astype(float), gamma.astype(float)
                info["nt"][here] = nt.astype(float)
            unfit = good_index & ~fits
            for k, par in enumerate(parameters):
                moved_p = np.isin(frame[p, SURFACE], list(par["ids"]))
                named_p = np.isin(frame[p, SURFACE], list(par["index_ids"]))
                u = velocity(par, moved_p, xp)
                dn = np.einsum("nab,nb->na", wp, dx[k, p] - u) + moved_normal(par, moved_p, np_)
                ddp, nu = dd[k, p], dnu[k, p]
                dnt = np.where(named_p & entered[p], LD(par["rate"]), LD(0))
                with np.errstate(invalid="ignore", divide="ignore"):
                    dci = -(np.sum(dn * dp, axis=1) + np.sum(np_ * ddp, axis=1))
                    dmu = (nu - mu * dnt) / nt
                    dct = (mu * mu * ci * dci - mu * (1 - ci * ci) * dmu) / ct
                    dgamma = ci * dmu + mu * dci - dct
                    refracted = dmu[:, None] * dp + mu[:, None] * ddp + dgamma[:, None] * np_ + gamma[:, None] * dn
                    turn = np.sum(ddp * np_, axis=1) + np.sum(dp * dn, axis=1)
                    reflected = ddp - 2 * (turn[:, None] * np_ + np.sum(dp * np_, axis=1)[:, None] * dn)
                new_d = np.where(refract[:, None], refracted, np.where(reflect[:, None], reflected, ddp))
                start_d[k] = new_d
                start_o[k] = dx[k, p] + OFFSET * new_d
                new_nu[k] = np.where(refract, dnt, nu)
                if info is not None:
                    with np.errstate(invalid="ignore"):
                        info["dmu"][here] = np.maximum(info["dmu"][here], np.where(refract, np.abs(dmu), 0).astype(float))
            count["n_reflections"] += int(np.sum(ok & reflect & fits & ~bad_landing & ~unknown))
        lost_unknown = ok & unknown
        lost_invalid = ok & ~unknown & (bad_landing | bad_interface)
        lost_unfit = ok & ~unknown & ~bad_landing & ~bad_interface & unfit
        count["n_unknown"] += int(lost_unknown.sum())
        count["n_invalid"] += int(lost_invalid.sum())
        count["n_unfit"] += int(lost_unfit.sum())
        good = ok & ~unknown & ~bad_landing & ~bad_interface & ~unfit
        for k, par in enumerate(parameters):
            u = velocity(par, np.isin(frame[here, SURFACE], list(par["ids"])), x)
            reach = start_o[k] + t[:, None] * start_d[k]
            with np.errstate(invalid="ignore", divide="ignore"):
                dt = np.sum(n * (u - reach), axis=1) / nd
            landed = reach + d * dt[:, None]
            dx[k, here] = np.where(good[:, None], landed, np.nan)
            dd[k, here] = np.where(good[:, None], start_d[k], np.nan)
            dnu[k, here] = new_nu[k]
        alive[here] = good
        entered[here] = enters
        if info is not None:
            info["nd"][here], info["t"][here] = nd.astype(float), t.astype(float)
            info["kappa"][here] = np.sqrt(np.sum(w_op * w_op, axis=(1, 2))).astype(float)
        normals[here], curvature[here] = n, w_op
        order = np.argsort(ids, kind="stable")
        previous = (ids[order], here[order])
    return dx, dd, count


def jacobian(frame, table, parameters):
    return trace_tangents(frame, table, parameters)[0]

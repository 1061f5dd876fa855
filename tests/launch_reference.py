"""Launch and wavelength sensitivities in numpy ``longdouble``: what DeviceFrame.sensitivity computes for a mix that holds a
SourceMotion or a WavelengthChange, restated from the formulas of include/prt.h and not from the kernel.  The normals and
Hessians are tests/sensitivity_reference.py's, the general velocity and the normal of a deformed surface
tests/design_reference.py's, the wavefront terms and sums tests/opd_sensitivity_reference.py's (``wavefront``, ``sums`` and
``statistics`` there take the dict ``trace`` returns here).  What is new here:

  the seed     in generation 0, for a launch parameter whose id range [lo, hi) holds the ray:  do = v + w x (o - c),
               dd = w x d;  0 for every other ray and parameter;
  dispersion   at a refraction that ENTERS a Sellmeier glass (b1, b2, b3, c1, c2, c3), wl the wavelength of the ray's row
               in the glass, in micrometres:
                   n^2 = 1 + sum_i b_i wl^2 / (wl^2 - c_i),   dn/dlambda = -(sum_i b_i c_i wl / (wl^2 - c_i)^2) / n
               and dnt = rate * dn/dlambda for a wavelength parameter whose range holds the ray (0 on leaving, and for a
               glass of constant index);
  dL           dL = dL_prev + dnu len + n d.(dx - do) with the seeded do in generation 0.

A parameter is design_reference's dict with four more keys: ``lo``, ``hi`` (the id range), ``seed`` (bool: the twist v, w,
c moves the launch of those rays) and ``colour`` (the wavelength rate, 0.0 for none).  ``glasses``: {surface id: (kind,
coef[6])} from a SceneSnapshot (``glasses_of``)."""
import numpy as np

import design_reference as dref
import opd_sensitivity_reference as oref  # noqa: F401  (wavefront, sums, statistics, default_sphere: used through this module)
import sensitivity_reference as sref
from sensitivity_reference import EPS_DIR, GEN, ID, INDEX, LD, OFFSET, SURFACE, TILT, X0, X1, group_sums, table_of, unpack  # noqa: F401

WAVELENGTH = 2
SELLMEIER = 4


def parameter(p):
    """The dict of any of pyrayt_amd's five kinds of parameter."""
    name = type(p).__name__
    if name in ("SourceMotion", "WavelengthChange"):
        lo, hi = p.id_range
        out = dict(v=np.zeros(3), w=np.zeros(3), c=np.zeros(3), S=np.zeros((3, 3)), ids=set(), rate=0.0, index_ids=set(),
                   lo=float(lo), hi=float(hi), seed=name == "SourceMotion", colour=0.0)
        if out["seed"]:
            out.update(v=np.asarray(p.translate, dtype=float), w=np.asarray(p.rotate, dtype=float),
                       c=np.asarray(p.pivot, dtype=float))
        else:
            out["colour"] = float(p.rate)
        return out
    return dict(dref.parameter(p), lo=0.0, hi=0.0, seed=False, colour=0.0)


def glasses_of(snapshot):
    prims, mats = snapshot.prims, snapshot.materials
    return {int(p["surface_id"]): (int(mats[p["material"]]["kind"]), np.array(mats[p["material"]]["coef"], dtype=float))
            for p in prims}


def dispersion(coef, wavelength):
    """dn/dlambda of a Sellmeier glass at the wavelengths (micrometres), and its index n."""
    b, c = np.asarray(coef[:3], dtype=LD), np.asarray(coef[3:], dtype=LD)
    wl = np.asarray(wavelength, dtype=LD)
    w2 = wl * wl
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(1 + sum(b[i] * w2 / (w2 - c[i]) for i in range(3)))
        return -sum(b[i] * c[i] * wl / (w2 - c[i]) ** 2 for i in range(3)) / n, n


def trace(frame, table, parameters, glasses, info=None):
    """dx, dd (K, R, 3), dnu, dL (K, R), the counters and each row's previous row, as a dict; NaN in dx, dd and dL where
    the ray cannot be followed.  ``info``, if a dict, gets the per-row geometry the error budget of
    tests/test_gpu_launch_sensitivity.py needs (design_reference's, and ``seed``, ``dndl``, ``dmu_size``, ``length``)."""
    frame = np.asarray(frame, dtype=float)
    wide = frame.astype(LD)
    rows, K = len(frame), len(parameters)
    dx = np.full((K, rows, 3), np.nan, dtype=LD)
    dd = np.full((K, rows, 3), np.nan, dtype=LD)
    dnu = np.zeros((K, rows), dtype=LD)
    dL = np.full((K, rows), np.nan, dtype=LD)
    alive = np.zeros(rows, dtype=bool)
    entered = np.zeros(rows, dtype=bool)
    count = {"n_unknown": 0, "n_invalid": 0, "n_unfit": 0, "n_reflections": 0}
    generations = frame[:, GEN].astype(int)
    previous = None
    before_row = np.full(rows, -1)
    normals = np.full((rows, 3), np.nan, dtype=LD)
    curvature = np.zeros((rows, 3, 3), dtype=LD)
    run = wide[:, X1] - wide[:, X0]
    length = np.sqrt(np.sum(run * run, axis=1))
    named = [(frame[:, ID] >= par["lo"]) & (frame[:, ID] < par["hi"]) for par in parameters]
    if info is not None:
        info.update(previous=before_row, nd=np.full(rows, np.nan), t=np.zeros(rows), kappa=np.zeros(rows),
                    conditioning=np.ones(rows), kind=np.zeros(rows, dtype=int), mu=np.ones(rows), ct=np.ones(rows),
                    gamma=np.zeros(rows), nt=np.ones(rows), dmu=np.zeros(rows), dmu_size=np.zeros(rows), seed=np.zeros(rows),
                    dndl=np.zeros(rows),
                    length=length.astype(float))
    for g in range(generations.max() + 1 if rows else 0):
        here = np.flatnonzero(generations == g)
        ids = frame[here, ID]
        o, x, d = wide[here, X0], wide[here, X1], sref._unit(wide[here, TILT])
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
                n[at], w_op[at] = sref.surface_normals(table[int(sid)], x[at], d[at], cond)
                raw, _ = sref.surface_normals(table[int(sid)], x[at], np.zeros_like(d[at]))  # (d = 0: never turned)
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
        path_before = np.zeros((K, len(here)), dtype=LD)
        ok = np.ones(len(here), dtype=bool)
        unfit = np.zeros(len(here), dtype=bool)
        bad_interface = np.zeros(len(here), dtype=bool)
        if g == 0:
            for k, par in enumerate(parameters):
                if par["seed"]:
                    v, w, c = (np.asarray(par[key], dtype=LD) for key in ("v", "w", "c"))
                    on = named[k][here][:, None]
                    start_o[k] = np.where(on, v + np.cross(w, o - c), LD(0))
                    start_d[k] = np.where(on, np.cross(w, d), LD(0))
                    if info is not None:
                        size = np.sqrt(np.sum(start_o[k] ** 2, axis=1)) + np.sqrt(np.sum(start_d[k] ** 2, axis=1))
                        info["seed"][here] = np.maximum(info["seed"][here], np.nan_to_num(size.astype(float)))
        else:
            sorted_ids, sorted_rows = previous
            where = np.minimum(np.searchsorted(sorted_ids, ids), len(sorted_ids) - 1)
            assert np.array_equal(sorted_ids[where], ids), "a ray has a row in a generation and none in the one before"
            p = sorted_rows[where]
            before_row[here] = p
            ok = alive[p].copy()
            dp, np_, wp, xp = sref._unit(wide[p, TILT]), normals[p], curvature[p], wide[p, X1]
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
            unfit = good_index & ~fits
            # dn/dlambda of the glass behind the previous row's surface, at this row's wavelength, where the ray enters it
            dndl = np.zeros(len(here), dtype=LD)
            for sid in np.unique(frame[p, SURFACE]):
                kind, coef = glasses.get(int(sid), (0, None)) if sid == int(sid) else (0, None)
                if kind == SELLMEIER:
                    at = (frame[p, SURFACE] == sid) & entered[p] & refract
                    dndl[at] = dispersion(coef, wide[here, WAVELENGTH][at])[0]
            if info is not None:
                info["kind"][here] = np.where(refract, 1, np.where(reflect, 2, 0))
                info["mu"][here], info["ct"][here], info["gamma"][here] = mu.astype(float), ct.astype(float), gamma.astype(float)
                info["nt"][here] = nt.astype(float)
                info["dndl"][here] = np.nan_to_num(np.abs(dndl).astype(float))
            for k, par in enumerate(parameters):
                moved_p = np.isin(frame[p, SURFACE], list(par["ids"]))
                named_p = np.isin(frame[p, SURFACE], list(par["index_ids"]))
                u = dref.velocity(par, moved_p, xp)
                dn = np.einsum("nab,nb->na", wp, dx[k, p] - u) + dref.moved_normal(par, moved_p, np_)
                ddp, nu = dd[k, p], dnu[k, p]
                dnt = np.where(named_p & entered[p], LD(par["rate"]), LD(0))
                if par["colour"]:
                    dnt = np.where(named[k][here] & entered[p], LD(par["colour"]) * dndl, LD(0))
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
                path_before[k] = dL[k, p]
                if info is not None:
                    with np.errstate(invalid="ignore"):
                        info["dmu"][here] = np.maximum(info["dmu"][here], np.where(refract, np.abs(dmu), 0).astype(float))
                        apart = (np.abs(nu) + mu * np.abs(dnt)) / nt  # (dmu's two terms before they cancel)
                        info["dmu_size"][here] = np.maximum(info["dmu_size"][here], np.where(refract, apart, 0).astype(float))
            count["n_reflections"] += int(np.sum(ok & reflect & fits & ~bad_landing & ~unknown))
        lost_unknown = ok & unknown
        lost_invalid = ok & ~unknown & (bad_landing | bad_interface)
        lost_unfit = ok & ~unknown & ~bad_landing & ~bad_interface & unfit
        count["n_unknown"] += int(lost_unknown.sum())
        count["n_invalid"] += int(lost_invalid.sum())
        count["n_unfit"] += int(lost_unfit.sum())
        good = ok & ~unknown & ~bad_landing & ~bad_interface & ~unfit
        for k, par in enumerate(parameters):
            u = dref.velocity(par, np.isin(frame[here, SURFACE], list(par["ids"])), x)
            reach = start_o[k] + t[:, None] * start_d[k]
            with np.errstate(invalid="ignore", divide="ignore"):
                dt = np.sum(n * (u - reach), axis=1) / nd
                landed = reach + d * dt[:, None]
                path = path_before[k] + new_nu[k] * length[here] + wide[here, INDEX] * np.sum(d * (landed - start_o[k]), axis=1)
            dx[k, here] = np.where(good[:, None], landed, np.nan)
            dd[k, here] = np.where(good[:, None], start_d[k], np.nan)
            dL[k, here] = np.where(good, path, np.nan)
            dnu[k, here] = new_nu[k]
        alive[here] = good
        entered[here] = enters
        if info is not None:
            info["nd"][here], info["t"][here] = nd.astype(float), t.astype(float)
            info["kappa"][here] = np.sqrt(np.sum(w_op * w_op, axis=(1, 2))).astype(float)
        normals[here], curvature[here] = n, w_op
        order = np.argsort(ids, kind="stable")
        previous = (ids[order], here[order])
    return dict(dx=dx, dd=dd, dnu=dnu, dL=dL, count=count, previous=before_row)


def focus_shift(x, d, w, axis):
    """The plane shift along the unit ``axis`` that minimises the weighted mean square radius about the centroid, rays
    continued as straight lines: -cov(p, s) / var(s), p the landing point and s = d / (d.a), both across the axis."""
    x, d, w, a = (np.asarray(v, dtype=LD) for v in (x, d, w, axis))
    a = a / np.sqrt(np.sum(a * a))
    across = np.eye(3, dtype=LD) - np.outer(a, a)
    p, s = x @ across, (d / (d @ a)[:, None]) @ across
    pc, sc = p - (w[:, None] * p).sum(axis=0) / w.sum(), s - (w[:, None] * s).sum(axis=0) / w.sum()
    return -(w * np.sum(pc * sc, axis=1)).sum() / (w * np.sum(sc * sc, axis=1)).sum()


def focus_gradient(x, d, w, dx, dd, axis):
    """(K,): the derivative of ``focus_shift`` for the tangents dx, dd (K, n, 3) of unit directions d."""
    x, d, w, a, dx, dd = (np.asarray(v, dtype=LD) for v in (x, d, w, axis, dx, dd))
    a = a / np.sqrt(np.sum(a * a))
    across = np.eye(3, dtype=LD) - np.outer(a, a)
    da = d @ a
    p, s = x @ across, (d / da[:, None]) @ across
    dp = dx @ across
    ds = (dd / da[None, :, None] - d[None] * ((dd @ a) / (da * da))[:, :, None]) @ across
    total = w.sum()
    pc, sc = p - (w[:, None] * p).sum(axis=0) / total, s - (w[:, None] * s).sum(axis=0) / total
    cov, var = (w * np.sum(pc * sc, axis=1)).sum() / total, (w * np.sum(sc * sc, axis=1)).sum() / total
    dcov = (w * (np.sum(dp * sc, axis=2) + np.sum(ds * pc, axis=2))).sum(axis=1) / total
    dvar = 2 * (w * np.sum(ds * sc, axis=2)).sum(axis=1) / total
    return -(dcov * var - cov * dvar) / (var * var)

"""Differential ray tracing in numpy ``longdouble``: what DeviceFrame.sensitivity computes, restated from the formulas of
include/prt.h and not from the kernel.  The join by ray id is an argsort / searchsorted per generation; the five
primitives' normals and Hessians are written out here a second time on purpose (the kernel takes them from the trace's own
device functions), so a slip in either shows as a difference.

A frame is an (R, 15) array in the column order of the result frame, generation-major.  A surface table is a dict
``id -> (type, normal_scale, params[6], minv[16])``; ``table_of`` makes one from a SceneSnapshot's ``prims``.  A parameter
is ``(v, w, c, ids)``: the twist and the surface ids it moves."""
import numpy as np

LD = np.longdouble
GEN, INTENSITY, INDEX, ID, SURFACE = 0, 1, 3, 4, 5
X0, X1, TILT = slice(6, 9), slice(9, 12), slice(12, 15)
SPHERE, CYLINDER, PLANE, CUBE, PARABOLOID = range(5)
EPS_DIR = LD(1e-12)
OFFSET = LD(1e-6)


def table_of(prims):
    return {int(p["surface_id"]): (int(p["type"]), int(p["normal_scale"]), np.array(p["params"], dtype=float),
                                   np.array(p["minv"], dtype=float).reshape(4, 4)) for p in prims}


def parameter(motion):
    """(v, w, c, ids) of a pyrayt_amd.Motion."""
    return (motion.translate, motion.rotate, motion.pivot, set(motion.surface_ids))


def _close(a, b):
    return np.abs(a - b) <= 1e-8 + 1e-5 * np.abs(b)  # (np.isclose's defaults, which the primitives use)


def gradient_and_hessian(kind, params, l):
    """Half the gradient g (n, 3) of the primitive's implicit function at the object points l (n, 3), and the diagonal
    (3,) of half its Hessian per point (n, 3): zero on planes, cube faces and end caps."""
    n = len(l)
    g = np.zeros((n, 3), dtype=LD)
    h = np.zeros((n, 3), dtype=LD)
    if kind == SPHERE:
        g[:] = l
        h[:] = 1
    elif kind == CYLINDER:
        g[:, 0], g[:, 1] = l[:, 0], l[:, 1]
        h[:, :2] = 1
        for cap, sign in ((params[1], -1.0), (params[2], 1.0)):
            on = _close(l[:, 2], cap)
            g[on] = (0, 0, sign)
            h[on] = 0
    elif kind == PLANE:
        g[:, 2] = 1
    elif kind == CUBE:
        for c in range(3):
            g[:, c] = np.where(_close(l[:, c], params[2 * c + 1]), 1.0, np.where(_close(l[:, c], params[2 * c]), -1.0, 0.0))
    elif kind == PARABOLOID:
        g[:, 0], g[:, 1], g[:, 2] = l[:, 0], l[:, 1], -2 * LD(params[0])
        h[:, :2] = 1
        on = _close(l[:, 2], params[1])
        g[on] = (0, 0, 1)
        h[on] = 0
    else:
        raise ValueError(kind)
    return g, h


def surface_normals(entry, x, d, conditioning=None):
    """At the world points x (n, 3) of a surface met along d (n, 3): the unit normal turned against d (n, 3) and the
    operator W (n, 3, 3) with dn = W (dx - u) for a point that slides on the surface."""
    kind, scale, params, minv = entry
    a = np.asarray(minv[:3, :3], dtype=LD)
    b = np.asarray(minv[:3, 3], dtype=LD)
    l = x @ a.T + b
    g, h = gradient_and_hessian(kind, params, l)
    w = g @ a  # A^T g
    length = np.sqrt(np.sum(w * w, axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = scale * w / length[:, None]
        m = np.einsum("ra,nr,rb->nab", a, h, a) / length[:, None, None]  # A^T H A / |A^T g|
        project = np.eye(3, dtype=LD) - n[:, :, None] * n[:, None, :]
        big_w = scale * np.einsum("nab,nbc->nac", project, m)
    flip = np.sum(n * d, axis=1) > 0
    n[flip] = -n[flip]
    big_w[flip] = -big_w[flip]
    if conditioning is not None:  # (how much of the object point A x + b cancels, against the gradient's length)
        with np.errstate(invalid="ignore", divide="ignore"):
            size = np.sqrt(np.sum(a * a)) * np.sqrt(np.sum(x * x, axis=1)) + np.sqrt(np.sum(b * b))
            conditioning[:] = np.maximum(1, size / np.sqrt(np.sum(g * g, axis=1))).astype(float)
    return n, big_w


def _velocity(par, moved, x):
    v, w, c, _ = par
    u = np.asarray(v, dtype=LD) + np.cross(np.asarray(w, dtype=LD), x - np.asarray(c, dtype=LD))
    return np.where(moved[:, None], u, LD(0))


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(np.sum(v * v, axis=1))[:, None]


def trace_tangents(frame, table, parameters, info=None):
    """dx (K, R, 3): d(landing point)/d(parameter) of every row, NaN where the ray cannot be followed; dd (K, R, 3): the
    derivative of the row's direction; a dict of the counters."""
    frame = np.asarray(frame, dtype=float)
    wide = frame.astype(LD)
    rows, K = len(frame), len(parameters)
    dx = np.full((K, rows, 3), np.nan, dtype=LD)
    dd = np.full((K, rows, 3), np.nan, dtype=LD)
    alive = np.zeros(rows, dtype=bool)
    count = {"n_unknown": 0, "n_invalid": 0, "n_unfit": 0, "n_reflections": 0}
    generations = frame[:, GEN].astype(int)
    previous = None  # (sorted ids, their rows) of the generation before
    normals = np.full((rows, 3), np.nan, dtype=LD)
    curvature = np.zeros((rows, 3, 3), dtype=LD)
    if info is not None:  # (per row, for the error budget of tests/test_gpu_sensitivity.py)
        info.update(previous=np.full(rows, -1), nd=np.full(rows, np.nan), t=np.zeros(rows), kappa=np.zeros(rows),
                    conditioning=np.ones(rows), kind=np.zeros(rows, dtype=int), mu=np.ones(rows), ct=np.ones(rows),
                    gamma=np.zeros(rows))
    for g in range(generations.max() + 1 if rows else 0):
        here = np.flatnonzero(generations == g)
        ids = frame[here, ID]
        o, x, d = wide[here, X0], wide[here, X1], _unit(wide[here, TILT])
        t = np.sum((x - o) * d, axis=1)
        # the landing's geometry
        n = np.full((len(here), 3), np.nan, dtype=LD)
        w_op = np.zeros((len(here), 3, 3), dtype=LD)
        known = np.zeros(len(here), dtype=bool)
        for sid in np.unique(frame[here, SURFACE]):
            at = frame[here, SURFACE] == sid
            if int(sid) in table and sid == int(sid):
                known[at] = True
                cond = np.ones(int(at.sum()))
                n[at], w_op[at] = surface_normals(table[int(sid)], x[at], d[at], cond)
                if info is not None:
                    info["conditioning"][here[at]] = cond
        finite = np.all(np.isfinite(frame[here][:, [6, 7, 8, 9, 10, 11, 12, 13, 14]]), axis=1) & np.all(np.isfinite(d), axis=1)
        nd = np.sum(n * d, axis=1)
        with np.errstate(invalid="ignore"):
            bad_landing = ~finite | (known & ~(nd < 0))
        unknown = finite & ~known
        # the ray's previous row
        start_o = np.zeros((K, len(here), 3), dtype=LD)
        start_d = np.zeros((K, len(here), 3), dtype=LD)
        ok = np.ones(len(here), dtype=bool)
        unfit = np.zeros(len(here), dtype=bool)
        bad_interface = np.zeros(len(here), dtype=bool)
        if g > 0:
            sorted_ids, sorted_rows = previous
            where = np.searchsorted(sorted_ids, ids)
            where = np.minimum(where, len(sorted_ids) - 1)
            assert np.array_equal(sorted_ids[where], ids), "a ray has a row in a generation and none in the one before"
            p = sorted_rows[where]
            ok = alive[p].copy()
            dp, np_, wp, xp = _unit(wide[p, TILT]), normals[p], curvature[p], wide[p, X1]
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
            unfit = good_index & ~fits
            moved_p = [np.isin(frame[p, SURFACE], list(par[3])) for par in parameters]
            for k, par in enumerate(parameters):
                u = _velocity(par, moved_p[k], xp)
                dn = np.einsum("nab,nb->na", wp, dx[k, p] - u)
                dn = dn + np.where(moved_p[k][:, None], np.cross(np.asarray(par[1], dtype=LD), np_), LD(0))
                ddp = dd[k, p]
                with np.errstate(invalid="ignore", divide="ignore"):
                    dci = -(np.sum(dn * dp, axis=1) + np.sum(np_ * ddp, axis=1))
                    dct = mu * mu * ci * dci / ct
                    refracted = mu[:, None] * ddp + (mu * dci - dct)[:, None] * np_ + gamma[:, None] * dn
                    turn = np.sum(ddp * np_, axis=1) + np.sum(dp * dn, axis=1)
                    reflected = ddp - 2 * (turn[:, None] * np_ + np.sum(dp * np_, axis=1)[:, None] * dn)
                new_d = np.where(refract[:, None], refracted, np.where(reflect[:, None], reflected, ddp))
                start_d[k] = new_d
                start_o[k] = dx[k, p] + OFFSET * new_d
            count["n_reflections"] += int(np.sum(ok & reflect & fits & ~bad_landing & ~unknown))
        # each ray is counted once, where it is lost
        lost_unknown = ok & unknown
        lost_invalid = ok & ~unknown & (bad_landing | bad_interface)
        lost_unfit = ok & ~unknown & ~bad_landing & ~bad_interface & unfit
        count["n_unknown"] += int(lost_unknown.sum())
        count["n_invalid"] += int(lost_invalid.sum())
        count["n_unfit"] += int(lost_unfit.sum())
        good = ok & ~unknown & ~bad_landing & ~bad_interface & ~unfit
        moved = [np.isin(frame[here, SURFACE], list(par[3])) for par in parameters]
        for k, par in enumerate(parameters):
            u = _velocity(par, moved[k], x)
            reach = start_o[k] + t[:, None] * start_d[k]
            with np.errstate(invalid="ignore", divide="ignore"):
                dt = np.sum(n * (u - reach), axis=1) / nd
            landed = reach + d * dt[:, None]
            dx[k, here] = np.where(good[:, None], landed, np.nan)
            dd[k, here] = np.where(good[:, None], start_d[k], np.nan)
        alive[here] = good
        if info is not None:
            info["nd"][here], info["t"][here] = nd.astype(float), t.astype(float)
            info["kappa"][here] = np.sqrt(np.sum(w_op * w_op, axis=(1, 2))).astype(float)
        normals[here], curvature[here] = n, w_op
        order = np.argsort(ids, kind="stable")
        previous = (ids[order], here[order])
    return dx, dd, count


def jacobian(frame, table, parameters):
    return trace_tangents(frame, table, parameters)[0]


def group_sums(x, w, dx, pivot):
    """The sums of include/prt.h over rows that are finite throughout, in longdouble: x (n, 3), w (n,), dx (K, n, 3),
    pivot (3,).  Returns a dict; 'moments' is the full symmetric K x K matrix."""
    x, w, dx, pivot = (np.asarray(v, dtype=LD) for v in (x, w, dx, pivot))
    keep = np.isfinite(w) & np.all(np.isfinite(x), axis=1) & np.all(np.isfinite(dx), axis=(0, 2))
    x, w, dx = x[keep], w[keep], dx[:, keep]
    r = x - pivot
    return {
        "count": int(keep.sum()), "w": w.sum(), "wx": (w[:, None] * x).sum(axis=0), "wrr": (w * np.sum(r * r, axis=1)).sum(),
        "wd": np.einsum("n,knc->kc", w, dx), "wrd": np.einsum("n,nc,knc->k", w, r, dx),
        "moments": np.einsum("n,jnc,knc->jk", w, dx, dx),
    }


def unpack(sums_row, K):
    """One group's device sums as the dict ``group_sums`` returns."""
    s = np.asarray(sums_row, dtype=LD)
    lower = np.zeros((K, K), dtype=LD)
    lower[np.tril_indices(K)] = s[6 + 4 * K:]
    return {"count": int(s[0]), "w": s[1], "wx": s[2:5], "wrr": s[5], "wd": s[6:6 + 3 * K].reshape(K, 3),
            "wrd": s[6 + 3 * K:6 + 4 * K], "moments": lower + np.tril(lower, -1).T}


# ---- frames by hand ---------------------------------------------------------------------------------------------------------
def rigid(w, c, angle_scale=1.0, v=(0.0, 0.0, 0.0)):
    """The 4x4 world transform of a finite motion: rotation by |w| * angle_scale about the axis w through c (Rodrigues),
    then the translation v * angle_scale."""
    w = np.asarray(w, dtype=float) * angle_scale
    angle = np.linalg.norm(w)
    m = np.eye(4)
    if angle > 0:
        k = w / angle
        kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        m[:3, :3] = np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * (kx @ kx)
    c = np.asarray(c, dtype=float)
    m[:3, 3] = c - m[:3, :3] @ c + np.asarray(v, dtype=float) * angle_scale
    return m

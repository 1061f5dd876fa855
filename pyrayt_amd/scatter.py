"""Scatter analysis: stray light spawned from the frame by the surfaces' BSDF and traced again (no counterpart upstream).

``DeviceFrame.ghosts`` follows the specular reflections of refracting surfaces; ``DeviceFrame.scatter`` follows surface
scatter -- a baffle wall, a lens edge, a barrel or a stop is not black, and a polished surface scatters a small share of
what meets it into a wide lobe.  Every row that lands on a surface with a ``Scatter`` model sends ``rays_per_hit`` child
rays back into the half space it came from, drawn cosine-weighted over the hemisphere or towards a ``Target`` disk (the
imager: importance sampling, the mode that makes stray light affordable), each with the energy the BSDF gives its
direction.  One HIP pass over the frame (``prt_frame_scatter_count`` / ``prt_frame_scatter_emit``,
``csrc/prt_scatter.hpp``; include/prt.h states the definitions); ``RayTracer.trace_scatter`` runs trace -> scatter ->
trace and ranks what reaches the imager.  The children are ordered so that every (source, scattering surface) is a
"source" of the per-source passes through ``rays_per_source=stride, n_groups=n_groups``.

A model is evaluated on the host and tabulated: the device knows one form only, ``KNOTS + 1`` doubles uniform in
``sqrt(b / 2)``, ``b = |beta - beta0|`` in [0, 2], interpolated linearly -- the rule user-defined glasses and coating stacks
follow already."""
import numpy as np
import pandas as pd

from .ghosts import GhostRays, _listed

KNOTS, MAX_MODELS, MAX_SURFACES, MAX_BUCKETS, MAX_RAYS_PER_HIT = 1024, 16, 64, 65535, 64
_COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")


def knots(dtype=np.float64):
    """``b`` at the table's knots: ``2 (k / KNOTS)^2``, k = 0 .. KNOTS."""
    u = np.arange(KNOTS + 1, dtype=dtype) / dtype(KNOTS)
    return dtype(2) * u * u


def basis(n):
    """The orthonormal basis ``(t1, t2)`` of a unit vector (Duff et al. 2017), in the operation order of include/prt.h."""
    x, y, z = (np.float64(v) for v in n)
    sign = np.copysign(np.float64(1.0), z)
    a = np.float64(-1.0) / (sign + z)
    b = (x * y) * a
    sx = sign * x
    return np.array([1.0 + (sx * x) * a, sign * b, -sx]), np.array([b, sign + (y * y) * a, -y])


class Scatter:
    """A shift-invariant BSDF ``f(b)``, ``b = |beta - beta0|``: ``table`` (what the device interpolates), ``kind`` and
    ``parameters`` (what it was made of) and ``model`` (the function of ``b`` behind it, any float dtype)."""

    def __init__(self, model, kind, parameters):
        self.model, self.kind, self.parameters = model, kind, dict(parameters)
        with np.errstate(all="ignore"):
            table = np.asarray(model(knots()), dtype=np.float64)
        if table.shape != (KNOTS + 1,) or not np.all(np.isfinite(table) & (table >= 0.0)):
            raise ValueError(f"Scatter.{kind}: the BSDF is finite and >= 0 for every b in [0, 2]")
        self.table = np.ascontiguousarray(table)

    @classmethod
    def lambertian(cls, albedo):
        """``f = albedo / pi``."""
        albedo = float(albedo)
        if not 0.0 <= albedo <= 1.0:
            raise ValueError("Scatter.lambertian: albedo in [0, 1]")
        value = np.float64(albedo) / np.float64(np.pi)
        return cls(lambda b: np.full(np.shape(b), value, dtype=np.asarray(b).dtype), "lambertian", dict(albedo=albedo))

    @classmethod
    def harvey(cls, b0, l, s):
        """Harvey-Shack: ``f = b0 (1 + (b / l)^2)^(s / 2)`` (s < 0: the slope of the wing, l: the shoulder)."""
        b0, l, s = float(b0), float(l), float(s)
        if not (b0 >= 0.0 and l > 0.0 and np.isfinite([b0, l, s]).all()):
            raise ValueError("Scatter.harvey: b0 >= 0, l > 0, all finite")
        return cls(lambda b: b0 * (1 + (b / type(b.flat[0])(l)) ** 2) ** (type(b.flat[0])(s) / 2), "harvey", dict(b0=b0, l=l, s=s))

    @classmethod
    def abg(cls, a, b, g):
        """ABg: ``f = a / (b + beta^g)``."""
        a, b_, g = float(a), float(b), float(g)
        if not (a >= 0.0 and b_ > 0.0 and np.isfinite([a, b_, g]).all()):
            raise ValueError("Scatter.abg: a >= 0, b > 0, all finite")
        return cls(lambda beta: a / (b_ + beta ** type(beta.flat[0])(g)), "abg", dict(a=a, b=b_, g=g))

    @classmethod
    def tabulated(cls, b, bsdf):
        """Measured data: ``bsdf`` at ascending ``b``, interpolated linearly in ``b`` (held constant past the ends)."""
        b, bsdf = np.asarray(b, dtype=np.float64), np.asarray(bsdf, dtype=np.float64)
        if b.ndim != 1 or b.shape != bsdf.shape or len(b) < 1 or not np.all(np.diff(b) > 0):
            raise ValueError("Scatter.tabulated: b ascending, one bsdf value each")
        return cls(lambda at: np.interp(np.asarray(at, dtype=np.float64), b, bsdf).astype(np.asarray(at).dtype),
                   "tabulated", dict(b=b, bsdf=bsdf))

    @classmethod
    def from_callable(cls, fn):
        """Any function of an array of ``b`` in [0, 2]."""
        return cls(lambda b: np.asarray(fn(b)), "callable", dict(fn=fn))

    def lookup(self, b):
        """The table at ``b`` as the device reads it (float64, the operations of include/prt.h)."""
        b = np.asarray(b, dtype=np.float64)
        q = np.sqrt(0.5 * b) * np.float64(KNOTS)
        k = np.where(q < KNOTS - 1, q, KNOTS - 1).astype(np.int64)
        lo = self.table[k]
        return lo + (q - k.astype(np.float64)) * (self.table[k + 1] - lo)

    def tis(self, theta_i=0.0, order=96):
        """The total integrated scatter at the angle of incidence ``theta_i`` (radians): the integral of ``f cos`` over
        the hemisphere, which is the integral of ``f(|beta - beta0|)`` over the unit disk of ``beta``, ``beta0 =
        sin(theta_i)`` -- Gauss-Legendre in ``sqrt(distance)`` and angle about ``beta0``, so that a peak there is
        resolved.  A Lambertian's is its albedo, in closed form."""
        if self.kind == "lambertian":
            return self.parameters["albedo"]
        s0 = float(np.sin(theta_i))
        x, w = np.polynomial.legendre.leggauss(order)
        phi, w_phi = np.pi * (x + 1.0), np.pi * w
        t, w_t = 0.5 * (x + 1.0), 0.5 * w  # (rho = rho_max(phi) t^2: d rho = 2 rho_max t dt)
        cos, sin = np.cos(phi), np.sin(phi)
        reach = -s0 * cos + np.sqrt(np.maximum(0.0, 1.0 - (s0 * sin) ** 2))  # (the disk's edge seen from beta0)
        rho = reach[:, None] * (t * t)[None, :]
        f = np.asarray(self.model(rho.ravel()), dtype=np.float64).reshape(rho.shape)
        return float(np.sum(w_phi[:, None] * w_t[None, :] * f * rho * 2.0 * reach[:, None] * t[None, :]))

    def table_error(self):
        """The largest relative deviation of the interpolated table from the model at the knots' midpoints (in u),
        in ``longdouble``."""
        wide = np.longdouble
        u = (np.arange(KNOTS, dtype=wide) + wide(0.5)) / wide(KNOTS)
        want = np.asarray(self.model(wide(2) * u * u), dtype=wide)
        table = self.table.astype(wide)
        got = table[:-1] + wide(0.5) * (table[1:] - table[:-1])
        with np.errstate(all="ignore"):
            deviation = np.where(want != 0, np.abs(got - want) / np.abs(want), np.abs(got - want))
        return float(deviation.max())

    def __repr__(self):
        shown = {k: v for k, v in self.parameters.items() if np.ndim(v) == 0 and not callable(v)}
        return f"Scatter.{self.kind}({', '.join(f'{k}={v!r}' for k, v in shown.items())})"


class Target:
    """Where the children are sent: ``Target.disk(centre, normal, radius)``."""

    def __init__(self, centre, normal, radius):
        self.centre, self.normal, self.radius = centre, normal, radius
        self.e1, self.e2 = basis(normal)

    @classmethod
    def disk(cls, centre, normal, radius):
        centre, normal, radius = np.asarray(centre, dtype=np.float64), np.asarray(normal, dtype=np.float64), float(radius)
        if centre.shape != (3,) or normal.shape != (3,) or not (np.isfinite(centre).all() and np.isfinite(normal).all()):
            raise ValueError("Target.disk: centre and normal are three finite numbers each")
        length = float(np.sqrt(np.sum(normal * normal)))
        if not length > 0.0:
            raise ValueError("Target.disk: the normal has no direction")
        if not (np.isfinite(radius) and radius > 0.0):
            raise ValueError("Target.disk: radius finite and > 0")
        return cls(centre, normal / length, radius)

    def packed(self):
        """The 13 doubles of include/prt.h: centre, normal, e1, e2, radius."""
        return np.ascontiguousarray(np.concatenate([self.centre, self.normal, self.e1, self.e2, [self.radius]]), dtype=np.float64)


class ScatterRays(GhostRays):
    """What ``DeviceFrame.scatter`` returns: the interface of ``GhostRays`` -- ``rays``, ``parent_row``, ``keys`` (per
    group ``(source, surface)``), ``stride``, ``n_groups``, ``counts``, ``bucket``, ``surfaces``, ``trace(scene_or_tracer)``
    -- and ``child`` (per child its number among its row's ``rays_per_hit``, device int32), ``models`` (per listed
    surface its ``Scatter``), ``toward``, ``rays_per_hit``, ``seed`` and the counters ``n_spawned``, ``n_rejected`` (samples
    outside the unit disk), ``n_below`` (the target point is below the surface's horizon), ``n_dark`` (no energy),
    ``n_dropped`` (below ``min_intensity``) and ``n_invalid`` (a child with a component that is not finite)."""

    def __init__(self, frame, rays, parent_row, child, counts, record, surfaces, ray_offset, models, toward, rays_per_hit, seed):
        self._children(frame, rays, parent_row, counts, surfaces, ray_offset)
        self.child, self.models, self.toward, self.rays_per_hit, self.seed = child, tuple(models), toward, rays_per_hit, seed
        (self.n_spawned, self.n_rejected, self.n_below, self.n_dark, self.n_dropped, self.n_invalid) = (int(v) for v in record[:6])


def _models(models):
    """``(surface ids, model number per id, the distinct Scatter objects)`` of a ``{surfaces: Scatter}`` dict."""
    if not isinstance(models, dict) or not models:
        raise ValueError("scatter: models is a dict {surface | component | tuple of them: Scatter}, not empty")
    ids, numbers, distinct = [], [], []
    for key, model in models.items():
        if not isinstance(model, Scatter):
            raise ValueError(f"scatter: the model of {key!r} is not a Scatter")
        if not any(model is known for known in distinct):
            distinct.append(model)
        number = next(k for k, known in enumerate(distinct) if model is known)
        for sid in _listed(key):
            if sid in ids:
                raise ValueError(f"scatter: surface {sid} has two models")
            ids.append(sid)
            numbers.append(number)
    if len(ids) > MAX_SURFACES:
        raise ValueError(f"scatter: at most {MAX_SURFACES} surfaces (got {len(ids)})")
    if len(distinct) > MAX_MODELS:
        raise ValueError(f"scatter: at most {MAX_MODELS} models a call (got {len(distinct)})")
    return ids, numbers, distinct


def _primitives(system, ids):
    from .scene import PRIM_DTYPE, SceneSnapshot

    if system is None:
        raise ValueError("scatter: system= (the components, a tracer or a SceneSnapshot) gives the surfaces' normals")
    if hasattr(system, "get_system"):
        system = system.get_system()
    snapshot = system if hasattr(system, "prims") else SceneSnapshot(system)
    prims = np.sort(np.asarray(snapshot.prims, dtype=PRIM_DTYPE), order="surface_id")
    if len(np.unique(prims["surface_id"])) != len(prims):
        raise ValueError("scatter: a surface id repeats in system")
    missing = sorted(set(ids) - set(int(v) for v in prims["surface_id"]))
    if missing:
        raise ValueError(f"scatter: surfaces that are not in system: {missing}")
    return np.ascontiguousarray(prims)


def spawn(frame, models, system, toward=None, rays_per_hit=1, seed=0, rays_per_source=None, n_groups=None,
          min_intensity=0.0, ray_offset=1e-6):
    """``DeviceFrame.scatter``: see there."""
    import torch

    from . import engine
    from .frame import _row_head

    try:
        frame._need(*_COLUMNS)
    except KeyError as error:
        raise ValueError(f"scatter: {error.args[0]}") from None
    ids, numbers, distinct = _models(models)
    if toward is not None and not isinstance(toward, Target):
        raise ValueError("scatter: toward is None (the hemisphere) or a Target (Target.disk(centre, normal, radius))")
    if isinstance(rays_per_hit, bool) or not isinstance(rays_per_hit, (int, np.integer)) or not 1 <= rays_per_hit <= MAX_RAYS_PER_HIT:
        raise ValueError(f"scatter: rays_per_hit is an integer in [1, {MAX_RAYS_PER_HIT}] (got {rays_per_hit!r})")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError("scatter: seed is an integer in [0, 2^64)")
    min_intensity, ray_offset = float(min_intensity), float(ray_offset)
    if not (np.isfinite(min_intensity) and min_intensity >= 0.0 and np.isfinite(ray_offset)):
        raise ValueError("scatter: min_intensity is finite and >= 0, ray_offset finite")
    prims = _primitives(system, ids)
    rows = frame._contiguous_rows()
    dev = rows.device
    n_rows = rows.shape[1]
    if n_rows * int(rays_per_hit) >= 2 ** 31 - 1:
        raise ValueError(f"scatter: rows x rays_per_hit below 2^31 (got {n_rows} x {rays_per_hit})")
    if rays_per_source:
        if n_groups is None:
            n_groups = max(1, int(frame._top_id() // rays_per_source) + 1)
    else:
        n_groups = 1
    n_groups = int(n_groups)
    n_buckets = n_groups * len(ids)
    if n_groups < 1 or n_buckets > MAX_BUCKETS:
        raise ValueError(f"scatter: at most {MAX_BUCKETS} buckets, groups x surfaces (got {n_groups} x {len(ids)})")
    tables = np.ascontiguousarray(np.stack([model.table for model in distinct]), dtype=np.float64)
    listed = np.ascontiguousarray(ids, dtype=np.int64)
    of = np.ascontiguousarray(numbers, dtype=np.int32)
    target = None if toward is None else toward.packed()
    counts = np.zeros(n_buckets, dtype=np.int64)
    record = np.zeros(8, dtype=np.int64)
    lib = engine.library()
    size = (n_rows, int(rays_per_hit), n_buckets, len(distinct))
    work = torch.empty(int(engine._check(lib.prt_frame_scatter_count_workspace_bytes(*size))), dtype=torch.uint8,
                       device=dev)  # (kept: the emit reads what the count left there)
    head = _row_head(rows)
    engine.call("prt_frame_scatter_count", *head, prims, len(prims), listed, of, len(listed), tables, len(distinct), target,
                int(rays_per_hit), int(seed), float(rays_per_source or 0), n_groups, min_intensity, ray_offset, counts,
                record, work.data_ptr(), device=dev)
    n_children = int(counts.sum())
    rays = torch.empty((engine.RAY_ROWS, n_children), dtype=torch.float64, device=dev)
    parent_row = torch.empty(n_children, dtype=torch.int64, device=dev)
    child = torch.empty(n_children, dtype=torch.int32, device=dev)
    if n_children:
        engine.call("prt_frame_scatter_emit", *head, int(rays_per_hit), n_buckets, len(distinct), n_children, work.data_ptr(),
                    rays, n_children, parent_row, child, device=dev, size=size[:3])
    return ScatterRays(frame, rays, parent_row, child, counts, record, ids, ray_offset, [distinct[k] for k in numbers],
                       toward, int(rays_per_hit), int(seed))


# ---- trace -> scatter -> trace -------------------------------------------------------------------------------------------
class ScatterAnalysis:
    """What ``RayTracer.trace_scatter`` returns.  ``frame``: the signal's frame (Fresnel losses applied when asked for);
    ``rays``: the ``ScatterRays`` spawned from it; ``scattered``: the children's frame; ``imager``: the surface id the
    table looks at; ``rays_per_source`` and ``n_sources`` of the tracer."""

    def __init__(self, frame, rays, scattered, imager, rays_per_source, n_sources):
        self.frame, self.rays, self.scattered, self.imager = frame, rays, scattered, int(imager)
        self.rays_per_source, self.n_sources = int(rays_per_source), int(n_sources)

    @staticmethod
    def _on(frame, imager, rays_per_source, n_groups):
        stats = frame.group_stats(surface=imager, rays_per_source=rays_per_source or None, n_groups=n_groups)
        return stats[stats["count"] > 0]

    def signal_energy(self):
        """The energy of the signal on the imager."""
        stats = self._on(self.frame, self.imager, self.rays_per_source, self.n_sources)
        return float((stats["count"] * stats["intensity"]).sum())

    def table(self):
        """One line per (source, scattering surface) that reaches the imager, the worst first: ``source``, ``surface``,
        ``rays``, ``energy`` (the sum of the children's intensities on the imager), ``share`` (of the signal's energy
        there), the centroid ``y``, ``z`` and ``rms_radius``."""
        columns = ["source", "surface", "rays", "energy", "share", "y", "z", "rms_radius"]
        lines = []
        if len(self.scattered):
            signal = self.signal_energy()
            for group, line in self._on(self.scattered, self.imager, self.rays.stride, self.rays.n_groups).iterrows():
                source, surface = (int(v) for v in self.rays.keys[int(group)])
                energy = float(line["count"] * line["intensity"])
                lines.append(dict(source=source, surface=surface, rays=int(line["count"]), energy=energy,
                                  share=energy / signal if signal > 0 else float("nan"), y=float(line["y"]),
                                  z=float(line["z"]), rms_radius=float(line["rms_radius"])))
        table = pd.DataFrame(lines, columns=columns)
        return table.sort_values("energy", ascending=False, kind="stable").reset_index(drop=True)

    def total_share(self):
        """The scattered energy on the imager over the signal's energy there."""
        return float(self.table()["share"].sum())

    def image(self, bins=64, range=None):
        """The scattered light on the imager: the intensity-weighted ``histogram2d`` of ``y1``, ``z1`` of the children's
        frame -- ``(image, y_edges, z_edges)``.  ``range`` must be given."""
        if range is None:
            raise ValueError("ScatterAnalysis.image: range=((y_lo, y_hi), (z_lo, z_hi)) is needed")
        if len(self.scattered) == 0:
            return None, None, None
        return self.scattered.histogram2d("y1", "z1", bins=bins, range=range, weights="intensity", surface=self.imager)[:3]


def trace_scatter(tracer, imager, models, toward=None, rays_per_hit=1, seed=0, fresnel=None, min_share=0.0):
    """``RayTracer.trace_scatter``: see there."""
    from . import distributed as _dist
    from .frame import _surface_id

    if tracer._gather == "none" and _dist.resolve_group(tracer._group) is not None:
        raise NotImplementedError("trace_scatter() of a sharded trace (gather='none') is not supported yet")
    if getattr(getattr(tracer._device_scene(), "snapshot", None), "host_surfaces", None):
        raise TypeError("trace_scatter: the scene has a material with a user-defined trace()")
    min_share = float(min_share)
    if not (np.isfinite(min_share) and min_share >= 0.0):
        raise ValueError("trace_scatter: min_share is finite and >= 0")
    kept = (tracer._frame, tracer._device_frame, tracer._simulation_complete, getattr(tracer, "_active_plan", None),
            tracer._record_surfaces, getattr(tracer, "_record_columns", None))
    try:
        tracer._record_surfaces, tracer._record_columns = (), None
        frame = tracer._run(to_host=False, plan=None)
    finally:
        (tracer._frame, tracer._device_frame, tracer._simulation_complete, tracer._active_plan, tracer._record_surfaces,
         tracer._record_columns) = kept
    n0 = frame.rows_per_generation[0] if frame.rows_per_generation else 0
    launch = float(frame["intensity"][:n0].max()) if n0 else 0.0
    options = None if fresnel is None else dict(fresnel)
    if options is not None:
        frame = frame.fresnel(**options).apply()
        options.pop("polarization", None)  # (children start unpolarised)
    rays_per_source, n_sources = tracer.get_rays_per_source(), len(tracer._sources)
    children = spawn(frame, models, tracer, toward=toward, rays_per_hit=rays_per_hit, seed=seed,
                     rays_per_source=rays_per_source or None, n_groups=n_sources, min_intensity=min_share * launch,
                     ray_offset=tracer.ray_offset_value)
    scattered = children.trace(tracer)
    if options is not None and len(scattered):
        scattered = scattered.fresnel(**options).apply()
    return ScatterAnalysis(frame, children, scattered, _surface_id(imager), rays_per_source, n_sources)

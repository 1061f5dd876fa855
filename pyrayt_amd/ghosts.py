"""Ghost analysis: Fresnel reflections spawned from the frame and traced again (no counterpart upstream).

``DeviceFrame.fresnel`` says how much energy every refracting surface takes from a ray; ``DeviceFrame.ghosts`` turns
that energy into child rays -- one reflected ray per refraction at the surfaces listed, an ordinary (13, n) ray set,
spawned by one HIP pass over the frame (``prt_frame_ghosts_count`` / ``prt_frame_ghosts_emit``, ``csrc/prt_ghosts.hpp``;
include/prt.h states the definitions) -- and ``RayTracer.trace_ghosts`` runs the rounds fresnel -> ghosts -> trace and
ranks what reaches the imager.  The children are ordered so that every (parent group, surface) is a "source" of the
per-source passes (``group_stats``, ``histogram2d``, ``enclosed_energy``, ``mtf``, ``paths``) through
``rays_per_source=stride, n_groups=n_groups``.

An interface is seen through two consecutive rows of a ray.  A ray that leaves the system has no later row, so the
reflection at the end of its last row is not seen: such rows are counted (``n_open``), and ``housing()`` gives the
absorbing sphere that ends every ray on a surface.  Children start unpolarised in their own Fresnel pass."""
import numpy as np
import pandas as pd

MAX_SURFACES, MAX_BUCKETS = 64, 65535  # (GHOST_MAX_SURFACES, GHOST_MAX_BUCKETS of csrc/prt_ghosts.hpp)
_COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")


def housing(radius, centre=(0.0, 0.0, 0.0)):
    """An absorbing sphere of ``radius`` about ``centre``, to be traced with the system: every ray then ends on a
    surface, every interface is followed by a row, and no row is open."""
    from . import g3d, materials

    return g3d.Sphere(float(radius), material=materials.absorber).move(*(float(c) for c in centre))


def refracting_surfaces(system):
    """The ids of every surface of a refracting material, ascending: ``system`` is a ``SceneSnapshot``, a ``RayTracer``
    or components."""
    from . import materials
    from .scene import SceneSnapshot

    if hasattr(system, "get_system"):
        system = system.get_system()
    snapshot = system if hasattr(system, "prims") and hasattr(system, "materials") else SceneSnapshot(system)
    kinds = np.asarray(snapshot.materials["kind"])[np.asarray(snapshot.prims["material"], dtype=np.int64)]
    glass = np.isin(kinds, (materials.CONST_INDEX, materials.SELLMEIER, materials.TABLE))
    return sorted(set(int(s) for s in np.asarray(snapshot.prims["surface_id"])[glass]))


def _listed(surfaces):
    """Surface ids in the order given (ids, objects with ``get_id()``, components with ``surface_ids``), each once."""
    if isinstance(surfaces, (str, bytes)) or hasattr(surfaces, "get_id") or hasattr(surfaces, "surface_ids") or \
            not hasattr(surfaces, "__iter__"):
        surfaces = (surfaces,)
    out = []
    for item in surfaces:
        ids = [sid for sid, _ in item.surface_ids] if hasattr(item, "surface_ids") else \
            [item.get_id() if hasattr(item, "get_id") else item]
        out += [int(sid) for sid in ids if int(sid) not in out]
    return out


def _absorbing_layers(coating, wavelengths):
    """Whether a layer of the coating has a complex index on any of the wavelengths."""
    if not coating.layers:
        return False
    return bool(np.any(coating.table(wavelengths)[1:1 + len(coating.layers)].imag != 0.0))


class GhostRays:
    """What ``DeviceFrame.ghosts`` returns.  ``rays``: the children, a device (13, n) ray set in the order of their
    groups; ``parent_row``: per child the row of the frame it was spawned at the end of (device int64); ``keys``:
    per group ``(parent group, surface)``, a host (n_groups, 2) int64 array; ``stride`` and ``n_groups``: a child's id
    is ``group * stride + rank``, so ``rays_per_source=stride, n_groups=n_groups`` makes every ghost path a source of
    the per-source passes of the children's frame; ``counts``: the children of every bucket (parent group x surface);
    ``surfaces``: the list spawned at; the counters ``n_spawned``, ``n_dropped`` (below ``min_intensity``), ``n_dark``
    (no energy reflected), ``n_invalid`` (a child with a component that is not finite) and ``n_open`` (rows that end
    on a listed surface and have no successor: their reflections are not seen)."""

    def __init__(self, frame, rays, parent_row, counts, record, surfaces, ray_offset):
        self._children(frame, rays, parent_row, counts, surfaces, ray_offset)
        self.n_spawned, self.n_dropped, self.n_dark, self.n_invalid, self.n_open = (int(v) for v in record[:5])

    def _children(self, frame, rays, parent_row, counts, surfaces, ray_offset):
        """The ray set, its buckets and its groups (what ``pyrayt_amd.scatter.ScatterRays`` has too)."""
        self.frame, self.rays, self.parent_row = frame, rays, parent_row
        self.counts, self.surfaces, self.ray_offset = np.asarray(counts, dtype=np.int64), tuple(surfaces), float(ray_offset)
        self.bucket = np.flatnonzero(self.counts > 0)
        self.n_groups = len(self.bucket)
        self.stride = int(self.counts.max()) if len(self.counts) else 0
        listed = np.asarray(self.surfaces, dtype=np.int64)
        self.keys = np.stack([self.bucket // max(len(listed), 1), listed[self.bucket % max(len(listed), 1)]],
                             axis=1).reshape(-1, 2)

    def __len__(self):
        return int(self.rays.shape[1])

    def trace(self, scene_or_tracer, generation_limit=None):
        """The children traced: a whole ``DeviceFrame``.  ``scene_or_tracer``: a ``RayTracer`` (its compiled scene, its
        generation limit unless one is given; its results and record settings are left alone) or an
        ``engine.DeviceScene`` (``generation_limit`` is then needed).  The rays start ``ray_offset`` off their surface
        already; the trace moves them on by the same offset after every later surface."""
        from . import engine
        from .frame import DeviceFrame

        torch = engine._torch()
        scene = scene_or_tracer._device_scene() if hasattr(scene_or_tracer, "_device_scene") else scene_or_tracer
        if generation_limit is None:
            if not hasattr(scene_or_tracer, "get_generation_limit"):
                raise ValueError(f"{type(self).__name__}.trace: generation_limit is needed with a DeviceScene")
            generation_limit = scene_or_tracer.get_generation_limit()
        if getattr(getattr(scene, "snapshot", None), "host_surfaces", None):
            raise TypeError(f"{type(self).__name__}.trace: the scene has a material with a user-defined trace()")
        if len(self) == 0:
            return DeviceFrame(torch.zeros((engine.RECORD_COLS, 0), dtype=torch.float64, device=self.rays.device), [0])
        rows, counts = scene.trace(self.rays, int(generation_limit), self.ray_offset, plan=None)
        return DeviceFrame(rows, counts or [0])


def spawn(frame, fresnel, surfaces=None, rays_per_source=None, n_groups=None, min_intensity=0.0, ray_offset=1e-6,
          system=None):
    """``DeviceFrame.ghosts``: see there."""
    import torch

    from . import engine
    from .frame import _INDEX, Fresnel, _lossless_ids, _row_head

    try:
        frame._need_whole("ghosts", columns=_COLUMNS)
    except KeyError as error:
        raise ValueError(f"ghosts: {error.args[0]}") from None
    if not isinstance(fresnel, Fresnel) or fresnel.frame is not frame or len(fresnel.transmittance) != len(frame):
        raise ValueError("ghosts: fresnel is the Fresnel of this very frame (frame.fresnel(...)), not of another one")
    if surfaces is None:
        if system is None:
            raise ValueError("ghosts: surfaces=None takes every refracting surface of system=, which is needed then")
        surfaces = refracting_surfaces(system)
    ids = _listed(surfaces)
    if len(ids) > MAX_SURFACES:
        raise ValueError(f"ghosts: at most {MAX_SURFACES} surfaces (got {len(ids)})")
    if not ids:
        raise ValueError("ghosts: no surface to spawn at")
    min_intensity, ray_offset = float(min_intensity), float(ray_offset)
    if not (np.isfinite(min_intensity) and min_intensity >= 0.0 and np.isfinite(ray_offset)):
        raise ValueError("ghosts: min_intensity is finite and >= 0, ray_offset finite")
    rows = frame._contiguous_rows()
    dev = rows.device
    n_rows = rows.shape[1]
    id0, n_ids, top = frame._id_range("ghosts", rows)
    if id0 >= 0.0:  # (groups are id // rays_per_source, as every per-source pass counts them: ids are taken from 0)
        id0, n_ids = 0.0, int(top) + 1
    if rays_per_source:
        if n_groups is None:
            n_groups = max(1, int((top - id0) // rays_per_source) + 1)
    else:
        n_groups = 1
    n_groups = int(n_groups)
    n_buckets = n_groups * len(ids)
    if n_groups < 1 or n_buckets > MAX_BUCKETS:
        raise ValueError(f"ghosts: at most {MAX_BUCKETS} buckets, groups x surfaces (got {n_groups} x {len(ids)})")
    for key, coating in (fresnel.coatings or {}).items():
        at = sorted(_lossless_ids(key) & set(ids))
        if at:
            wavelengths = np.zeros(0)
            if n_rows:
                wavelengths = engine.to_host(torch.unique(rows[_INDEX["wavelength"]])).astype(np.float64)
                wavelengths = wavelengths[np.isfinite(wavelengths) & (wavelengths > 0)]
            if _absorbing_layers(coating, wavelengths if len(wavelengths) else np.array([0.55])):
                raise ValueError(f"ghosts: the coating of surface {at[0]} has a layer of complex index: an absorbing "
                                 "stack reflects less than 1 - T, which is what the pass takes for R")
    transmittance = fresnel.transmittance.contiguous()
    counts = np.zeros(n_buckets, dtype=np.int64)
    record = np.zeros(8, dtype=np.int64)
    generations = np.ascontiguousarray(frame.rows_per_generation, dtype=np.int64)
    listed = np.ascontiguousarray(ids, dtype=np.int64)
    lib = engine.library()
    work = torch.empty(int(engine._check(lib.prt_frame_ghosts_count_workspace_bytes(n_rows, n_ids, n_buckets))),
                       dtype=torch.uint8, device=dev)  # (kept: the emit reads what the count left there)
    head = _row_head(rows)
    engine.call("prt_frame_ghosts_count", *head[:3], generations, len(generations), id0, n_ids, transmittance, listed,
                len(listed), float(rays_per_source or 0), n_groups, min_intensity, ray_offset, counts, record,
                work.data_ptr(), device=dev)
    n_children = int(counts.sum())
    rays = torch.empty((engine.RAY_ROWS, n_children), dtype=torch.float64, device=dev)
    parent_row = torch.empty(n_children, dtype=torch.int64, device=dev)
    if n_children:
        engine.call("prt_frame_ghosts_emit", *head, n_ids, transmittance, ray_offset, n_buckets, n_children,
                    work.data_ptr(), rays, n_children, parent_row, device=dev, size=(n_rows, n_buckets))
    return GhostRays(frame, rays, parent_row, counts, record, ids, ray_offset)


# ---- the rounds --------------------------------------------------------------------------------------------------------
class GhostOrder:
    """One order of a ``GhostAnalysis``: ``ghosts`` (the ``GhostRays`` it was traced from; None for order 0, the
    signal), ``frame`` (its trace) and ``fresnel`` (the Fresnel pass of that frame)."""

    def __init__(self, ghosts, frame, fresnel):
        self.ghosts, self.frame, self.fresnel = ghosts, frame, fresnel


class GhostAnalysis:
    """What ``RayTracer.trace_ghosts`` returns.  ``orders[k]``: the ``GhostOrder`` of order k; order 0 is the signal,
    order k >= 1 the rays that were reflected k times (an order without children ends the list).  ``imager``: the
    surface id the table looks at; ``rays_per_source`` and ``n_sources`` of the tracer."""

    def __init__(self, orders, imager, rays_per_source, n_sources):
        self.orders, self.imager = list(orders), int(imager)
        self.rays_per_source, self.n_sources = int(rays_per_source), int(n_sources)
        self._applied = {}

    def _grouping(self, order):
        if order == 0:
            return self.rays_per_source, self.n_sources
        return self.orders[order].ghosts.stride, self.orders[order].ghosts.n_groups

    def path(self, order, group):
        """``(surfaces, source)`` of group ``group`` of order ``order``: the surfaces its rays were reflected at, the
        first reflection first, and the source they left."""
        surfaces = []
        for k in range(order, 0, -1):
            group, surface = (int(v) for v in self.orders[k].ghosts.keys[group])
            surfaces.append(surface)
        return tuple(reversed(surfaces)), int(group)

    def frame(self, order):
        """The frame of an order with the Fresnel losses applied (``Fresnel.apply()``)."""
        if order not in self._applied:
            self._applied[order] = self.orders[order].fresnel.apply()
        return self._applied[order]

    def _stats(self, order):
        rays_per_source, n_groups = self._grouping(order)
        stats = self.frame(order).group_stats(surface=self.imager, rays_per_source=rays_per_source or None,
                                              n_groups=n_groups)
        return stats[stats["count"] > 0]

    def signal_energy(self):
        """The energy of the signal (order 0) on the imager, Fresnel losses applied."""
        stats = self._stats(0)
        return float((stats["count"] * stats["intensity"]).sum())

    def table(self):
        """One line per ghost path that reaches the imager, the worst first: ``order``, ``source``, ``surfaces`` (first
        reflection first), ``rays``, ``energy`` (the sum of the applied intensities on the imager), ``share`` (of the
        signal's energy there), the centroid ``y``, ``z`` and ``rms_radius``."""
        signal = self.signal_energy()
        lines = []
        for order in range(1, len(self.orders)):
            if len(self.orders[order].frame) == 0:
                continue
            for group, line in self._stats(order).iterrows():
                surfaces, source = self.path(order, int(group))
                energy = float(line["count"] * line["intensity"])
                lines.append(dict(order=order, source=source, surfaces=surfaces, rays=int(line["count"]), energy=energy,
                                  share=energy / signal if signal > 0 else float("nan"), y=float(line["y"]),
                                  z=float(line["z"]), rms_radius=float(line["rms_radius"])))
        table = pd.DataFrame(lines, columns=["order", "source", "surfaces", "rays", "energy", "share", "y", "z", "rms_radius"])
        return table.sort_values("energy", ascending=False, kind="stable").reset_index(drop=True)

    def image(self, bins=64, range=None):
        """The ghost image on the imager: the intensity-weighted ``histogram2d`` of ``y1``, ``z1`` summed over the
        orders >= 1 -- ``(image, y_edges, z_edges)``.  ``range`` must be given (one grid for every order)."""
        if range is None:
            raise ValueError("GhostAnalysis.image: range=((y_lo, y_hi), (z_lo, z_hi)) is needed, one grid for all orders")
        total, edges = None, None
        for order in np.arange(1, len(self.orders)):
            if len(self.orders[order].frame) == 0:
                continue
            hist, y_edges, z_edges = self.frame(int(order)).histogram2d("y1", "z1", bins=bins, range=range,
                                                                        weights="intensity", surface=self.imager)[:3]
            total, edges = hist if total is None else total + hist, (y_edges, z_edges)
        return (total, *edges) if total is not None else (None, None, None)


def trace_ghosts(tracer, imager, order=2, fresnel=None, surfaces=None, min_share=0.0, strict=True):
    """``RayTracer.trace_ghosts``: see there."""
    from . import distributed as _dist
    from .frame import _surface_id

    if tracer._gather == "none" and _dist.resolve_group(tracer._group) is not None:
        raise NotImplementedError("trace_ghosts() of a sharded trace (gather='none') is not supported yet")
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order < 1:
        raise ValueError(f"trace_ghosts: order is an integer >= 1 (got {order!r})")
    min_share = float(min_share)
    if not (np.isfinite(min_share) and min_share >= 0.0):
        raise ValueError("trace_ghosts: min_share is finite and >= 0")
    options = dict(fresnel or {})
    listed = refracting_surfaces(tracer) if surfaces is None else _listed(surfaces)
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
    rays_per_source, n_groups = tracer.get_rays_per_source(), len(tracer._sources)
    orders = [GhostOrder(None, frame, frame.fresnel(**options))]
    options.pop("polarization", None)  # (children start unpolarised: the parent's field is not carried across)
    for k in range(1, int(order) + 1):
        before = orders[-1]
        children = spawn(before.frame, before.fresnel, listed, rays_per_source=rays_per_source or None, n_groups=n_groups,
                         min_intensity=min_share * launch, ray_offset=tracer.ray_offset_value)
        if strict and children.n_open:
            raise ValueError(f"trace_ghosts: {children.n_open} rows of order {k - 1} end on a listed surface and are not "
                             "followed by another row -- their rays leave the system -- so the reflections there are "
                             "not seen; trace the system inside ghosts.housing(radius), or pass strict=False")
        if len(children) == 0:
            break
        frame = children.trace(tracer)
        orders.append(GhostOrder(children, frame, frame.fresnel(**options)))
        rays_per_source, n_groups = children.stride, children.n_groups
    return GhostAnalysis(orders, _surface_id(imager), tracer.get_rays_per_source(), len(tracer._sources))

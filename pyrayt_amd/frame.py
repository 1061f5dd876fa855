"""DeviceFrame: the trace result kept columnar in HBM.

``RayTracer.trace()`` returns a pandas DataFrame like the reference
(``pyrayt/_pyrayt.py:147-186``); for a 1M-ray trace that is a 360 MB device-to-host copy which
costs two orders of magnitude more than the trace itself.  ``RayTracer.trace_device()`` returns
this view instead: the engine's (15, R) record block, one contiguous row per column, with the
handful of selections the reference's examples make on the frame (``results.loc[results[
"surface"] == id]``, per-generation slices, spot statistics: ``examples/lens_design.ipynb``)
done on the device, so that only what is looked at crosses PCIe.  The grouped reductions
(``group_stats``: per-source / per-wavelength spot and focus statistics, the notebook's cells
11-16) are one HIP kernel over the column block (``prt_frame_reduce``, ``csrc/prt_frame.hpp``);
row selections that return a new frame are torch indexing -- plumbing around the result.
"""

from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pandas as pd

COLUMNS = ("generation", "intensity", "wavelength", "index", "id", "surface",
           "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")
_INDEX = {name: k for k, name in enumerate(COLUMNS)}


class DeviceFrame:
    def __init__(self, rows, rows_per_generation=None, columns=None):
        """rows: (15, R) tensor (device or host), generation-major.  columns: indices of the columns the trace wrote
        (a record plan with a column list, ``engine.RecordPlan(columns=...)``; None: all fifteen) -- the other rows of
        the block hold whatever was there and are never handed out."""
        assert rows.shape[0] == len(COLUMNS)
        self.rows = rows
        self.rows_per_generation = list(rows_per_generation or [])
        self.written = None if columns is None or len(columns) == len(COLUMNS) else tuple(sorted(columns))
        self.origin = None  # how the frame lost rows of its trace ("where", "select", "generation", "record_only"), if it did
        if self.written is not None:
            self.columns = tuple(COLUMNS[k] for k in self.written)  # (names of the columns THIS frame holds)

    # --- shape / access -----------------------------------------------------------------------
    columns = COLUMNS

    def __len__(self):
        return int(self.rows.shape[1])

    @property
    def shape(self):
        return (len(self), len(self.columns))

    def _need(self, *names):
        if self.written is not None:
            missing = [name for name in names if _INDEX[name] not in self.written]
            if missing:
                raise KeyError(f"this frame was recorded without the column(s) {missing} (RecordPlan(columns=...))")

    def __getitem__(self, column):
        """One column as a 1-D tensor view (no copy)."""
        self._need(column)
        return self.rows[_INDEX[column]]

    # --- selections ------------------------------------------------------------------------------
    def generation(self, g):
        """Rows of generation g: a contiguous slice (rows are generation-major), no kernel."""
        if g < len(self.rows_per_generation):
            start = sum(self.rows_per_generation[:g])
            part = DeviceFrame(self.rows[:, start:start + self.rows_per_generation[g]],
                               [0] * g + [self.rows_per_generation[g]], self.written)
            part.origin = "generation"
            return part
        return self.where(generation=g)

    def last_generation(self):
        """Rows of the highest generation in the frame -- the notebook's way to say "the rays that reached the imager"
        when the imager is not at hand (``examples/lens_design.ipynb`` cells 12, 15, 20:
        ``results.loc[results['generation'] == np.max(results['generation'])]``).  Rows are generation-major, so
        this is the frame's last slice: no kernel, no copy."""
        number = self.last_generation_number()
        return self if number is None else self.generation(number)

    def last_generation_number(self):
        """The highest generation that recorded rows (None for an empty frame)."""
        counts = self.rows_per_generation
        if counts:
            working = [g for g, k in enumerate(counts) if k]
            return working[-1] if working else None
        if len(self) == 0:
            return None
        return int(float(self["generation"].max()))

    def where(self, **equals):
        """Rows whose named columns equal the given values, e.g. where(surface=6, generation=2)."""
        mask = None
        for name, value in equals.items():
            m = self[name] == float(value)
            mask = m if mask is None else (mask & m)
        if mask is None:
            return self
        part = DeviceFrame(self.rows[:, mask], None, self.written)
        part.origin = "where"
        return part

    def select(self, mask):
        part = DeviceFrame(self.rows[:, mask], None, self.written)
        part.origin = "select"
        return part

    # --- reductions the notebook does on the frame -------------------------------------------------
    def group_stats(self, surface=None, generation=None, rays_per_source=None, n_groups=None, group=None, comm=None):
        """Per-source statistics of the rows that hit ``surface`` and / or belong to ``generation``
        (``examples/lens_design.ipynb`` cells 11-16: ``results.loc[results['surface'] == id]``
        grouped by ``source_id = id // rays_per_source``, ``_pyrayt.py:349-354``).

        Returns a DataFrame indexed by source id with columns ``count``, ``y`` / ``z`` (spot centroid
        of the end points), ``rms_radius`` (about that centroid), ``focus`` / ``focus_std`` (mean and
        spread of the x-axis intercepts ``x0 - x_tilt * y0 / y_tilt``, the notebook's paraxial-focus
        estimate), ``wavelength`` and ``intensity`` (means).  One library call (``prt_frame_stats``): the
        HIP reduction kernel runs twice, the second pass about the first pass's per-group means so that
        the second moments are well conditioned, and the final arithmetic happens on the device too.
        Without ``rays_per_source`` everything is one group.

        ``group`` (a ``torch.distributed`` group) or ``comm`` (a ``pyrayt_amd.distributed.LibraryComm``): this
        frame holds one rank's rows of a sharded trace (``RayTracer(..., gather="none")``) and the statistics
        wanted are those of the WHOLE frame.  Every rank reduces its own rows; the per-group sums -- nine doubles a
        group -- are added across the ranks (RCCL all-reduce inside the library with ``comm``; ``torch.distributed``
        with a group of another backend), once per pass.  Every rank gets the full statistics and the rows stay
        where they are: the alternative, re-assembling the frame, moves 315 MB into every GPU for a 1M-ray trace.
        Collective: every rank of the group calls it, with the same arguments (``n_groups`` included, or None)."""
        self._need("generation", "surface", "id", "intensity", "wavelength", "x0", "y0", "x_tilt", "y_tilt", "y1", "z1")
        sharded = group is not None or comm is not None
        if rays_per_source:
            if n_groups is None:
                top = float(self["id"].max()) if len(self) else -1.0
                if sharded:
                    top = _all_reduce_max(top, group, comm, self.rows.device)
                n_groups = max(1, int(top // rays_per_source) + 1)
        else:
            n_groups = 1
        stats = (self._stats_sharded(surface, generation, rays_per_source, n_groups, group, comm) if sharded
                 else self._stats(surface, generation, rays_per_source, n_groups))
        frame = pd.DataFrame({
            "count": stats[:, 0].astype(np.int64), "y": stats[:, 1], "z": stats[:, 2], "rms_radius": stats[:, 3],
            "focus": stats[:, 4], "focus_std": stats[:, 5], "wavelength": stats[:, 6], "intensity": stats[:, 7],
        })
        frame.index.name = "source_id"
        return frame

    def _stats(self, surface, generation, rays_per_source, n_groups):
        """``prt_frame_stats``: both reduction passes and the final arithmetic on the device, one
        (n_groups, 8) block brought to the host."""
        import torch

        from . import engine

        rows = self.rows
        if rows.stride(1) != 1:
            rows = rows.contiguous()
        out = torch.empty((n_groups, 8), dtype=torch.float64, device=rows.device)
        engine.call("prt_frame_stats", *_row_head(rows), *_row_filter(surface, generation, rays_per_source, n_groups), out,
                    device=rows.device, size=(n_groups,))
        return out.cpu().numpy()

    def _reduce_pass(self, surface, generation, rays_per_source, n_groups, pivots):
        """One pass of ``prt_frame_reduce`` over this frame's rows: the (n_groups, 9) sums, on the device."""
        import torch

        from . import engine

        rows = self._contiguous_rows()
        sums = torch.empty((n_groups, 9), dtype=torch.float64, device=rows.device)
        engine.call("prt_frame_reduce", *_row_head(rows), *_row_filter(surface, generation, rays_per_source, n_groups),
                    pivots, sums, device=rows.device)
        return sums

    def _stats_sharded(self, surface, generation, rays_per_source, n_groups, group, comm):
        """The whole frame's statistics from this rank's rows (see ``group_stats``)."""
        import torch

        from . import engine

        if comm is not None:  # one library call: both passes, two ncclAllReduce of (n_groups, 9) doubles
            rows = self._contiguous_rows()
            out = torch.empty((n_groups, 8), dtype=torch.float64, device=rows.device)
            engine.call("prt_frame_stats_sharded", comm._handle, *_row_head(rows)[1:],
                        *_row_filter(surface, generation, rays_per_source, n_groups), out, device=rows.device,
                        size=(n_groups,), sized_by="prt_frame_stats")
            return out.cpu().numpy()
        # another transport adds the sums: the passes and the two small steps are separate library calls
        sums = _all_reduce_sum(self._reduce_pass(surface, generation, rays_per_source, n_groups, None), group)
        pivots = self._pivots(sums, n_groups)
        sums = _all_reduce_sum(self._reduce_pass(surface, generation, rays_per_source, n_groups, pivots), group)
        return self._finish(sums, pivots, n_groups).cpu().numpy()

    def _pivots(self, sums, n_groups):
        """``prt_frame_pivots``: per group the means a second pass accumulates about, (n_groups, 3) on the device."""
        import torch

        from . import engine

        pivots = torch.empty((n_groups, 3), dtype=torch.float64, device=sums.device)
        engine.call("prt_frame_pivots", sums.device.index or 0, sums, n_groups, pivots, device=sums.device)
        return pivots

    def _finish(self, sums, pivots, n_groups):
        """``prt_frame_finish``: a second pass's sums and its pivots -> the (n_groups, 8) statistics, on the device."""
        import torch

        from . import engine

        out = torch.empty((n_groups, 8), dtype=torch.float64, device=sums.device)
        engine.call("prt_frame_finish", sums.device.index or 0, sums, pivots, n_groups, out, device=sums.device)
        return out

    def mean_square(self, quantity, about=0.0, transform=None, surface=None, generation=None, rays_per_source=None,
                    n_groups=None, group=None):
        """``np.mean(np.square(f(rows) - about))`` -- the shape of every merit function in the lens-design notebook --
        as one HIP reduction over the column block (``prt_frame_mean_square``), nothing but the result crossing PCIe.

        quantity: a column name, or ``"axis_intercept"`` for ``x0 - x_tilt * y0 / y_tilt`` (the notebook's paraxial
        focus, cells 12 / 15); transform: None or ``"sin"``; surface / generation filter the rows as in
        ``group_stats`` (``generation="last"``: the highest generation, cells 12 / 15 / 20).  Examples:
        the coma metric of cell 20, ``np.mean(np.square(np.sin(ray_set['y_tilt']) - np.sin(angle)))``, is
        ``frame.mean_square("y_tilt", about=np.sin(angle), transform="sin", generation="last")``; the focus error
        of cells 28 / 32 is ``frame.mean_square("axis_intercept", about=system_focus, generation="last")``.
        Rows whose value is not finite are skipped, like pandas' mean skips NaN.

        Returns a float, or with ``rays_per_source`` a DataFrame indexed by source id (``count``, ``mean`` of
        f(rows) - about, ``mean_square``).  ``group`` (a ``torch.distributed`` group): this frame is one rank's
        share of a sharded trace; the three sums per source are added across the ranks before dividing."""
        import torch

        from . import engine

        column = 15 if quantity == "axis_intercept" else _INDEX[quantity]
        how = {None: 0, "sin": 1}[transform]
        self._need("generation", "surface", "id", *(("x0", "y0", "x_tilt", "y_tilt") if column == 15 else (quantity,)))
        if generation == "last":
            generation = self.last_generation_number()
            if group is not None:
                generation = int(_all_reduce_max(-1.0 if generation is None else float(generation), group, None,
                                                 self.rows.device))
            if generation is None or generation < 0:
                generation = 0
        if rays_per_source:
            if n_groups is None:
                top = float(self["id"].max()) if len(self) else -1.0
                if group is not None:
                    top = _all_reduce_max(top, group, None, self.rows.device)
                n_groups = max(1, int(top // rays_per_source) + 1)
        else:
            n_groups = 1
        rows = self._contiguous_rows()
        sums = torch.empty((n_groups, 3), dtype=torch.float64, device=rows.device)
        engine.call("prt_frame_mean_square", *_row_head(rows), *_row_filter(surface, generation, rays_per_source, n_groups),
                    column, how, float(about), sums, device=rows.device)
        if group is not None:
            sums = _all_reduce_sum(sums, group)
        sums = sums.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            mean, mean_square = sums[:, 1] / sums[:, 0], sums[:, 2] / sums[:, 0]
        if not rays_per_source:
            return float(mean_square[0])
        frame = pd.DataFrame({"count": sums[:, 0].astype(np.int64), "mean": mean, "mean_square": mean_square})
        frame.index.name = "source_id"
        return frame

    # --- histograms (examples/lens_design.ipynb cell 19: ``ray_set.hist('y1')``; spot diagrams, irradiance maps) --------
    def histogram(self, x, bins=10, range=None, weights=None, density=False, surface=None, generation=None,
                  rays_per_source=None, n_groups=None, group=None):
        """``np.histogram`` of one quantity of the selected rows, binned on the device (``prt_frame_histogram``): returns
        ``(hist, edges)`` as float64 numpy arrays, equal to numpy's -- counts exactly.

        x: a column name or ``"axis_intercept"``; bins: an int or an edge array; range: ``(lo, hi)`` or None; weights:
        None or a column name (the sums are float64 adds: exact for integer weights such as the built-in sources'
        intensity 100, otherwise equal to numpy's up to the last bits); density: numpy's normalisation.  The edges are
        numpy's own (``np.histogram_bin_edges``), with numpy's ``ValueError``s; string estimators ("auto", "fd", ...)
        are not supported.  ``range=None`` with an int ``bins`` takes the range of the FINITE values of the selected
        rows (``prt_frame_range``): numpy raises for input with NaN or inf instead, and pandas' ``Series.hist`` drops the
        NaN first, which is what this matches; no finite value gives (0, 1), a single value v gives (v - 0.5, v + 0.5)
        as in numpy.  surface / generation select rows as in ``mean_square`` (``generation="last"``: the highest
        generation of this frame).  With ``rays_per_source`` the histogram gains a leading axis of ``n_groups`` groups
        (``id // rays_per_source``; default as in ``group_stats``).  ``group``: a ``torch.distributed`` group whose
        ranks each hold a share of the rows (a trace with ``gather="none"``): the automatic range is taken over every
        rank's rows and the counts and sums are added, so every rank gets the histogram of the whole frame."""
        hist, edges = self._histogram((x,), bins, range, weights, density, surface, generation, rays_per_source,
                                      n_groups, group)
        return hist, edges[0]

    def histogram2d(self, x, y, bins=10, range=None, weights=None, density=False, surface=None, generation=None,
                    rays_per_source=None, n_groups=None, group=None):
        """``np.histogram2d`` of two quantities of the selected rows (a spot diagram: ``"y1", "z1"``; weighted by
        ``"intensity"``, an irradiance map): returns ``(H, xedges, yedges)``, H of shape (nx, ny), or (n_groups, nx,
        ny) with ``rays_per_source``.  bins: an int, a pair of ints, an edge array, or a pair of edge arrays (or an
        int and an array); range: a pair of ``(lo, hi)``, either of which may be None (the finite range of that
        quantity, as in ``histogram``).  A row counts only when both of its values fall in a bin.  Everything else as
        in ``histogram``."""
        hist, edges = self._histogram((x, y), bins, range, weights, density, surface, generation, rays_per_source,
                                      n_groups, group)
        return hist, edges[0], edges[1]

    def _histogram(self, quantities, bins, range, weights, density, surface, generation, rays_per_source, n_groups,
                   group):
        import torch

        from . import engine

        codes = [15 if q == "axis_intercept" else _INDEX[q] for q in quantities]
        needed = [name for q in quantities for name in (("x0", "y0", "x_tilt", "y_tilt") if q == "axis_intercept" else (q,))]
        if weights is not None:
            needed.append(weights)
        if surface is not None:
            needed.append("surface")
        if rays_per_source:
            needed.append("id")
        self._need(*needed)
        frame = self
        if generation == "last":
            generation = self.last_generation_number()
            if group is not None:
                generation = int(_all_reduce_max(-1.0 if generation is None else float(generation), group, None,
                                                 self.rows.device))
            if generation is None or generation < 0:
                generation = 0
        if generation is not None:
            if self.rows_per_generation:  # (generation-major: one generation's rows are a slice, no filter needed)
                _, start, size = self._generation_slice(generation)
                frame = DeviceFrame(self.rows[:, start:start + size], None, self.written)
                generation = None
            else:
                self._need("generation")
        if rays_per_source:
            if n_groups is None:
                top = float(self["id"].max()) if len(self) else -1.0
                if group is not None:
                    top = _all_reduce_max(top, group, None, self.rows.device)
                n_groups = max(1, int(top // rays_per_source) + 1)
        else:
            n_groups = 1
        rows = frame._contiguous_rows()
        dev = rows.device
        head, which = _row_head(rows), _row_filter(surface, generation, rays_per_source, n_groups)
        surface, generation = which[:2]  # (as the passes read them: the range takes no groups)

        def finite_range(axis):
            box = torch.empty(2, dtype=torch.float64, device=dev)
            engine.call("prt_frame_range", *head, surface, generation, codes[axis], box, device=dev)
            if group is not None:
                box[1:].neg_()
                box = _all_reduce_min(box, group)
                box[1:].neg_()
            lo, hi = box.cpu().tolist()
            return (0.0, 1.0) if lo > hi else (lo, hi)

        edges, uniform = histogram_edges(bins, range, len(quantities), finite_range)
        nx = len(edges[0]) - 1
        ny = len(edges[1]) - 1 if len(edges) == 2 else 0
        shape = (n_groups, nx, max(ny, 1))
        counts = torch.empty(shape, dtype=torch.int64, device=dev)
        sums = torch.empty(shape, dtype=torch.float64, device=dev) if weights is not None else None
        engine.call("prt_frame_histogram", *head, *which, codes[0], edges[0], nx, int(uniform[0]),
                    codes[1] if ny else -1, edges[1] if ny else None, ny, int(ny and uniform[1]),
                    _weight_column(weights), counts, sums, device=dev, size=(n_groups, nx, ny, sums is not None))
        out = counts if sums is None else sums
        if group is not None:
            out = _all_reduce_sum(out, group)
        hist = out.cpu().numpy().astype(np.float64)
        if not ny:
            hist = hist[:, :, 0]
        if density:
            hist = np.stack([_density(h, edges) for h in hist])
        return (hist if rays_per_source else hist[0]), edges

    # --- optical path and wavefront error (no counterpart upstream) --------------------------------------------------
    def _need_whole(self, what, columns=None):
        """The optical path sums a ray's rows over every generation before the one looked at: the frame must be the
        whole frame of a trace."""
        if self.origin == "record_only":
            raise ValueError(f"{what} needs every surface's rows: this frame was recorded under record_only() / a record "
                             "plan that keeps some surfaces only (trace_wavefront() records what it needs)")
        if self.origin is not None:
            raise ValueError(f"{what} needs the whole frame of a trace: this frame was made by {self.origin}()")
        if not self.rows_per_generation or sum(self.rows_per_generation) != len(self):
            raise ValueError(f"{what} needs the whole frame of a trace: rows_per_generation is not known for this frame")
        self._need(*(columns or _PATH_COLUMNS))

    def _contiguous_rows(self):
        """The rows as the library reads them: contiguous along the row axis."""
        rows = self.rows
        return rows if rows.stride(1) == 1 or rows.shape[1] <= 1 else rows.contiguous()

    def _generation_slice(self, generation):
        """``(generation, start, size)``: the number of the generation ("last": the highest that recorded rows), where
        its rows begin in the generation-major block and how many they are -- none past the last generation."""
        if generation == "last":
            generation = self.last_generation_number() or 0
        size = self.rows_per_generation[int(generation)] if int(generation) < len(self.rows_per_generation) else 0
        return generation, sum(self.rows_per_generation[:int(generation)]), size

    def _id_range(self, what, rows):
        """``(id0, n_ids, top)``: the smallest id of ``rows``, the length of the dense per-id arrays of a join by ray id,
        the largest id; ``(0.0, 1, 0.0)`` for an empty frame."""
        import torch

        if rows.shape[1] == 0:
            return 0.0, 1, 0.0
        ids = rows[_INDEX["id"]]
        id0, top = (float(v) for v in torch.stack([ids.min(), ids.max()]).cpu())
        if not (np.isfinite(id0) and np.isfinite(top)):
            raise ValueError(f"{what}: an id is not an integer in the frame's id range")
        return id0, int(top - id0) + 1, top

    def _top_id(self):
        """The largest ray id of the frame (a host read), -1 for an empty frame: what ``_group_count`` counts from."""
        return float(self["id"].max()) if len(self) else -1.0

    def optical_path(self):
        """The cumulative optical path length of every row, a device tensor of ``len(self)`` float64: the row's segment
        ``index * sqrt(dx*dx + dy*dy + dz*dz)`` plus the cumulative OPL of the same ray's row in the previous generation
        (``prt_frame_optical_path``, one HIP launch per generation).  The rows are the contract: the 1e-6 relaunch
        offset of ``_pyrayt.py:449`` is part of ``x0`` as written.  Ids must be integers, unique within a generation.
        Needs the whole frame of a trace (not one made by ``where`` / ``select`` / ``generation``, nor under
        ``record_only``): ``ValueError`` otherwise."""
        self._need_whole("optical_path")
        return self._optical_path()

    def _optical_path(self):
        import torch

        from . import engine

        rows = self._contiguous_rows()
        dev = rows.device
        opl = torch.empty(rows.shape[1], dtype=torch.float64, device=dev)
        if rows.shape[1] == 0:
            return opl
        id0, n_ids, _ = self._id_range("optical_path", rows)
        counts = np.ascontiguousarray(self.rows_per_generation, dtype=np.int64)
        engine.call("prt_frame_optical_path", *_row_head(rows)[:3], counts, len(counts), id0, n_ids, opl, device=dev)
        return opl

    def wavefront(self, surface, reference="centroid", radius=None, axis=None, basis=None, pupil_radius=None,
                  zernike=15, weights=None, generation=None, rays_per_source=None, n_groups=None, group=None):
        """The wavefront error at ``surface`` (an id or an object with ``get_id()``; None: every row that passes
        ``generation``): per row the optical path difference against a reference sphere and the pupil point, per
        group (``id // rays_per_source``) its RMS, peak-to-valley and Zernike fit.  Returns a ``Wavefront``.

        Each selected row's ray is extended backwards from its end point Q along its direction to the sphere of centre
        P and radius R (``reference``: "centroid" -- the mean of the group's Q --, a point, or an (n_groups, 3) array;
        ``radius``: None -- the distance from P to the mean of the group's segment starts (x0, y0, z0) at the surface,
        a stand-in for the exit pupil --, a number or one per group).  OPD = the OPL there minus the group's pivot (the
        OPL there of its first row); a ray whose line misses the sphere has OPD NaN and counts in ``n_missed``.  The
        pupil point is E - P in the basis (e1, e2) of the plane perpendicular to ``axis`` (default: the x axis, this
        package's optical axis, with e1 = y and e2 = z; ``basis`` = (e1, e2) or None for one made from y / z),
        divided by ``pupil_radius`` (None: the group's largest radial extent).  ``zernike``: J <= 36 terms in Noll's
        order and RMS normalisation, fitted by least squares on the normal equations the device accumulates
        (``weights``: None or a column such as "intensity"); ``rank`` reports what the pupil fill can tell apart (a
        single ring of rays cannot tell piston from defocus).  Piston is removed from ``opd``, ``rms`` and ``pv``.
        Needs the whole frame of a trace, like ``optical_path``.  ``group=`` (sharded frames) is not supported yet."""
        if group is not None:
            raise NotImplementedError("wavefront() of a sharded frame (group=) is not supported yet")
        return self._wavefront(surface, reference, radius, axis, basis, pupil_radius, zernike, weights, generation,
                               rays_per_source, n_groups)[0]

    def _wavefront(self, surface, reference, radius, axis, basis, pupil_radius, zernike, weights, generation,
                   rays_per_source, n_groups):
        """``wavefront()``, and what the PSF passes read again: (Wavefront, the rows the passes ran on, the surface
        filter, n_groups, the group records on the device)."""
        import torch

        from . import engine

        terms = int(zernike)
        if terms != zernike or not 1 <= terms <= 36:
            raise ValueError(f"zernike: the number of terms, 1 to 36 (got {zernike!r})")
        _check_weights(weights)
        if pupil_radius is not None and not (np.isfinite(pupil_radius) and pupil_radius > 0):
            raise ValueError("pupil_radius: a positive number, or None for the group's largest radial extent")
        axes = pupil_axes(axis, basis)
        _check_reference_name(reference)
        surface_id = None if surface is None else float(_surface_id(surface))
        self._need_whole("wavefront")
        if weights is not None:
            self._need(weights)
        n_groups = _group_count(rays_per_source, n_groups, self._top_id)
        dev = self.rows.device
        centres = None if isinstance(reference, str) else _group_points(reference, n_groups, dev, "reference: a point")
        radii = None
        if radius is not None:
            radii = torch.as_tensor(np.broadcast_to(np.asarray(radius, dtype=float), (n_groups,)).copy()).to(dev)
        opl = self._optical_path()
        rows = self._contiguous_rows()
        if generation is not None:  # (generation-major: one generation's rows are a slice)
            generation, start, size = self._generation_slice(generation)
            rows, opl = rows[:, start:start + size], opl[start:start + size]
        n_rows = rows.shape[1]
        entries = terms * (terms + 1) // 2 + terms + 3
        opd = torch.empty(n_rows, dtype=torch.float64, device=dev)
        pupil = torch.empty((n_rows, 2), dtype=torch.float64, device=dev)
        record = torch.empty((n_groups, 12), dtype=torch.float64, device=dev)
        normal = torch.empty((n_groups, entries), dtype=torch.float64, device=dev)
        engine.call("prt_frame_wavefront", *_row_head(rows), opl, *_row_filter(surface_id, None, rays_per_source, n_groups),
                    centres, radii, axes, float(pupil_radius or 0.0), terms, _weight_column(weights), opd, pupil, record,
                    normal, device=dev, size=(n_rows, n_groups, terms, weights is not None))
        record_host = engine.host(record)
        normal_host = engine.host(normal)
        n_selected = int(record_host[:, 6].sum())
        wave = Wavefront(opd[:n_selected], pupil[:n_selected], record_host, normal_host, terms)
        # (what sensitivity(wavefront=) holds a Wavefront to: the frame, the selection, the weights and the pupil's basis)
        wave._made_of = dict(frame=self, surface=surface_id, generation=None if generation is None else int(generation),
                             rays_per_source=float(rays_per_source or 0), n_groups=n_groups, weights=weights, axes=axes)
        return wave, rows, surface_id, n_groups, record

    # --- diffraction PSF and Strehl ratio (no counterpart upstream) ---------------------------------------------------
    def psf(self, surface, *, world_unit_um, pixels=128, pixel_size=None, centre=(0.0, 0.0), weights="intensity",
            reference="centroid", radius=None, axis=None, basis=None, generation=None, rays_per_source=None,
            n_groups=None, group=None, fresnel=None, focus=None, track="chief"):
        """The diffraction image of a point at ``surface`` -- the Huygens PSF -- and its Strehl ratio, per group
        (``id // rays_per_source``).  Returns a ``PSF``.

        It runs ``wavefront()`` with the same reference-sphere arguments (``reference``, ``radius``, ``axis``,
        ``basis``, ``generation``, ``rays_per_source``, ``n_groups``) and then one HIP pass (``prt_frame_psf``): every ray
        that meets the reference sphere is a secondary source of amplitude ``sqrt(w)`` (``weights``: a column, default
        "intensity", or None for ones) and phase ``(OPD + d - R) / lambda``, summed at every pixel of a grid in the plane
        through P perpendicular to the axis; rays of one wavelength add coherently, wavelengths incoherently.  The
        image is normalised so that a perfect wave on the same rays gives 1 at P; ``strehl`` is the image at P
        (include/prt.h states the definitions).  world_unit_um: how many micrometres one world unit is (1000 for mm),
        required -- wavelengths are in micrometres.  pixels: an int or (nx, ny), 1..1024; pixel_size: a number or
        (du, dv) in world units, default lambda_min * F / 4 with F = R / (2 rho_max) the smallest over the groups with
        rays; centre: (u0, v0), the grid's centre in world units.  The wavelengths are the distinct values of the
        selected rows, at most 16.

        Sampling: each ray stands for an equal share of the pupil's area, or carries its share in ``weights``; random
        pupil samples leave a noise floor of about 1 / (number of rays) in the normalised image.  Obliquity and 1/r
        are taken as constant over the pupil (an error of order NA^2 at the rim).  Needs the whole frame of a trace,
        like ``wavefront``; ``group=`` (sharded frames) is not supported yet.

        ``fresnel``: None, or the ``Fresnel`` of this frame with its fields (``self.fresnel(fields=True, ...)``).  The
        sum is then the polarised one (``prt_frame_vector_psf``): every ray's amplitude is ``sqrt(w)`` times its complex
        field vector, projected on (e1, e2, a), so the image carries the coatings' phases, the rotation of the field
        across the pupil and its axial component besides the losses.  ``weights`` is read from this frame, not from
        ``fresnel.apply()``: the transmittance is in the fields already.  Polarised input has one state (Ea),
        unpolarised input two (Ea and Eb, added incoherently with weight 1/2).  The two states of
        ``fresnel(polarization=None)`` follow each ray's own direction, which serves the per-ray transmittance but is
        not a state of the beam; they are first turned into two states that are uniform across the beam
        (``Fresnel.uniform_states()``; ``VectorPSF.fresnel`` is the Fresnel that was summed).  A ``Fresnel`` built by
        hand is summed as it is.  Returns a ``VectorPSF``.

        ``focus``: None, or 1 to 256 finite shifts delta along the axis, in world units, with the sign of ``mtf(focus=)``
        and ``enclosed_energy(focus=)``: the image and the Strehl ratio on every plane through P + delta a, from the one
        wavefront and in one call (``prt_frame_psf_focus``) -- a Huygens sum can be evaluated anywhere, so a scan needs
        no re-trace.  Returns a ``PSFScan``.  The reference sphere stays where it is; the normalisation is that of
        ``focus=None`` on every plane, and the plane 0.0 has its bits.  ``track`` (read only with ``focus``): "chief" --
        each plane's grid is centred on the group's chief line, the line through P and the weighted mean of its rays'
        points on the reference sphere, so the image of an off-axis field stays on the grid --, or None -- every grid is
        centred at ``centre`` on the line through P parallel to the axis.  Not with ``fresnel=`` or ``group=``."""
        if focus is not None:
            if fresnel is not None or group is not None:
                raise ValueError("psf: focus= does not go with fresnel= or group= (the polarised sum and sharded "
                                 "frames have no through-focus pass yet)")
            if track is not None and track != "chief":
                raise ValueError(f'track: "chief" or None (got {track!r})')
            focus = _mtf_values(focus, "focus", 256, "finite shifts along the axis")
        import torch

        from . import engine

        if group is not None:
            raise NotImplementedError("psf() of a sharded frame (group=) is not supported yet")
        if fresnel is not None:
            if not isinstance(fresnel, Fresnel):
                raise ValueError(f"fresnel: None or the Fresnel of this frame (got {fresnel!r})")
            if fresnel.frame is not self:
                raise ValueError("psf: fresnel was computed on another frame (call this frame's fresnel(fields=True))")
            if fresnel.field is None:
                raise ValueError("psf: the fields were not kept (fresnel(fields=True))")
        unit = _positive(world_unit_um, "world_unit_um: how many micrometres one world unit is (1000 for mm)")
        nx, ny = _pixel_counts(pixels)
        step, uv0 = _pixel_grid(pixel_size, centre)
        _check_weights(weights)
        self._need_whole("psf")
        self._need("wavelength", *(() if weights is None else (weights,)))
        surface_id = None if surface is None else float(surface.get_id() if hasattr(surface, "get_id") else surface)
        wavelengths = self._psf_wavelengths(surface_id, generation)
        wave, rows, surface_id, n_groups, record = self._wavefront(
            surface_id, reference, radius, axis, basis, None, 15, weights, generation, rays_per_source, n_groups)
        f_number, step = _f_number_and_step(wave, wavelengths, unit, step, "psf")
        dev = rows.device
        n_rows = rows.shape[1]
        n_w = len(wavelengths)
        lam = np.ascontiguousarray(wavelengths, dtype=np.float64)
        uv0 = np.ascontiguousarray(uv0)
        opd = wave.opd if wave.opd.numel() else torch.empty(1, dtype=torch.float64, device=dev)
        pupil = wave.pupil if wave.pupil.numel() else torch.empty(2, dtype=torch.float64, device=dev)
        # the twenty leading arguments of the three Huygens sums, and what their results are told of the grid
        head = (*_row_head(rows), *_row_filter(surface_id, None, rays_per_source, n_groups), opd, pupil, record,
                _weight_column(weights), lam, n_w, unit, nx, ny, step[0], step[1], uv0)
        made = _HuygensGrid(wavelengths, unit, (nx, ny), step, (float(uv0[0]), float(uv0[1])), f_number, wave)
        if fresnel is not None:
            if fresnel.launch_states == "per_ray":  # (the pass's own two states: made uniform across the beam first)
                fresnel = fresnel.uniform_states()
            return self._vector_psf(fresnel, generation, rows, n_groups, head, made)
        if focus is not None:
            return self._psf_focus(focus, track, rows, n_groups, head, made)
        image = torch.empty((n_groups, n_w, nx, ny), dtype=torch.float64, device=dev)
        strehl = torch.empty(n_groups, dtype=torch.float64, device=dev)
        out = torch.empty((n_groups, n_w, 4), dtype=torch.float64, device=dev)
        engine.call("prt_frame_psf", *head, image, strehl, out, device=dev, size=(n_rows, n_groups, n_w))
        return PSF(engine.host(image), engine.host(strehl), engine.host(out), *made)

    def _psf_focus(self, focus, track, rows, n_groups, head, made):
        """``psf(focus=)`` after the wavefront (``head``, ``made``: see ``psf``): the call, and the ``PSFScan``."""
        import torch

        from . import engine

        wavelengths, (nx, ny), wave = made.wavelengths, made.pixels, made.wave
        dev, n_rows = rows.device, rows.shape[1]
        n_w, n_f = len(wavelengths), len(focus)
        image = torch.empty((n_groups, n_f, n_w, nx, ny), dtype=torch.float64, device=dev)
        strehl = torch.empty((n_groups, n_f), dtype=torch.float64, device=dev)
        out = torch.empty((n_groups, n_w, 4), dtype=torch.float64, device=dev)
        axial = torch.empty(max(n_rows, 1), dtype=torch.float64, device=dev)
        line = torch.empty((n_groups, 2), dtype=torch.float64, device=dev)
        centres = torch.empty((n_groups, n_f, 2), dtype=torch.float64, device=dev)
        axes = np.ascontiguousarray(wave._made_of["axes"], dtype=np.float64)
        engine.call("prt_frame_psf_focus", *head, axes, focus, n_f, 0 if track is None else 1, image, strehl, out, axial,
                    line, centres, device=dev, size=(n_rows, n_groups, n_w, n_f))
        return PSFScan(engine.host(image), engine.host(strehl), engine.host(out), axial[:wave.opd.numel()],
                       engine.host(line), engine.host(centres), focus, *made, track)

    def _vector_psf(self, fresnel, generation, rows, n_groups, head, made):
        """``psf(fresnel=)`` after the wavefront (``head``, ``made``: see ``psf``): the field planes as the library reads
        them, and the call."""
        import torch

        from . import engine

        wavelengths, (nx, ny), wave = made.wavelengths, made.pixels, made.wave
        dev, n_rows = rows.device, rows.shape[1]
        n_w = len(wavelengths)
        n_states = 1 if fresnel.polarization is not None else 2
        field = fresnel.field
        if tuple(field.shape) != (6, len(self)):
            raise ValueError(f"psf: fresnel.field is (6, {len(self)}) for this frame (got {tuple(field.shape)})")
        # (6, n) real as prt_frame_fresnel wrote it, or the real parts and then the imaginary parts of a complex one
        planes = torch.cat([field.real, field.imag]) if field.is_complex() else field
        planes = planes.to(dev, torch.float64).contiguous()
        start = 0
        if generation is not None:  # (the rows are that generation's slice: the planes are read from the same offset)
            start = self._generation_slice(generation)[1]
        field_ld = max(planes.shape[1], 1)
        stokes = torch.empty((n_groups, n_w, 5, nx, ny), dtype=torch.float64, device=dev)
        strehl = torch.empty((n_groups, 4), dtype=torch.float64, device=dev)
        out = torch.empty((n_groups, n_w, n_states, 6), dtype=torch.float64, device=dev)
        axes = np.ascontiguousarray(wave._made_of["axes"], dtype=np.float64)
        engine.call("prt_frame_vector_psf", *head, planes.data_ptr() + 8 * start if n_rows else None, field_ld,
                    int(planes.shape[0]), n_states, axes, stokes, strehl, out, device=dev,
                    size=(n_rows, n_groups, n_w, n_states))
        return VectorPSF(engine.host(stokes), engine.host(strehl), engine.host(out), *made, fresnel)

    def _psf_wavelengths(self, surface_id, generation):
        """The distinct wavelengths of the rows the wavefront selects (sorted), found where the rows are."""
        rows = self.rows
        if generation is not None:
            _, start, size = self._generation_slice(generation)
            rows = rows[:, start:start + size]
        lam = rows[_INDEX["wavelength"]]
        if surface_id is not None:
            lam = lam[rows[_INDEX["surface"]] == surface_id]
        if hasattr(lam, "unique"):
            values = lam.unique().cpu().numpy().astype(np.float64)
        else:
            values = np.unique(np.asarray(lam, dtype=np.float64))
        if not len(values):
            raise ValueError("psf: no row is selected at this surface")
        return _distinct_wavelengths(values, "psf")

    # --- what the image passes ask of their caller (mtf, enclosed_energy, ray_aberrations) -----------------------------
    def _image_selection(self, what, surface, generation, rays_per_source, n_groups, weights, whole=None):
        """``(surface_id, generation, n_groups)`` of a pass over the rows at ``surface``: the surface's id or None,
        "last" resolved, the groups counted from the largest ray id where ``n_groups`` is None.  The frame must hold
        the columns the pass reads -- ``whole``: the columns of a pass that joins by ray id and so needs the whole
        frame of a trace -- and ``weights`` must be None or a column."""
        _check_weights(weights)
        surface_id = None if surface is None else float(_surface_id(surface))
        needed = ([] if whole is not None else list(_MTF_COLUMNS)) + ([weights] if weights is not None else [])
        if whole is None:
            needed += (["id"] if rays_per_source else []) + (["surface"] if surface_id is not None else [])
            needed += ["generation"] if generation is not None else []
        try:
            if whole is not None:
                self._need_whole(what, whole)
            self._need(*needed)
        except KeyError as error:
            raise ValueError(f"{what}: {error.args[0]}") from None
        if generation == "last":
            generation = self.last_generation_number() or 0
        return surface_id, generation, int(_group_count(rays_per_source, n_groups, self._top_id))

    # --- geometric MTF through focus (no counterpart upstream) --------------------------------------------------------
    def mtf(self, surface, frequencies, *, azimuths=(0.0, 90.0), focus=(0.0,), reference="centroid", axis=None,
            basis=None, weights="intensity", generation=None, rays_per_source=None, n_groups=None, group=None):
        """The geometric MTF at ``surface`` (an id or an object with ``get_id()``; None: every row that passes
        ``generation``), per group (``id // rays_per_source``), at every focus shift, azimuth and frequency.  Returns
        an ``MTF``.

        Each ray's line, from its end point Q along its direction u, meets the plane through C + delta a perpendicular
        to the axis a at x(delta) = p + delta s in the basis (e1, e2) of that plane; the OTF is the weighted mean of
        exp(-2 pi i k.x(delta)) with k = nu (cos theta, sin theta), theta in degrees from e1 towards e2 and nu in cycles
        per world unit (include/prt.h states the definitions).  frequencies: 1 to 4096 values >= 0; azimuths: 1 to 16
        (default tangential and sagittal for a field along e1: 0 and 90); focus: 1 to 256 shifts delta along a, in
        world units.  reference: "centroid" (the weighted centroid of the group's end points) or a point or an
        (n_groups, 3) array; axis / basis as in ``wavefront``; weights: a column (default "intensity") or None for ones.
        Past the surface a ray is a straight line, so a through-focus scan needs no re-trace.  Rays whose direction is
        perpendicular to the axis, or with a value that is not finite, count in ``n_missed``.

        One HIP pass (``prt_frame_mtf``) over the rows it selects: it reads only end points, directions and the columns
        of the selection, so frames made by ``where``, ``select`` or under ``record_only`` work and give the same bits
        as the whole frame.  ``group=`` (sharded frames) is not supported yet."""
        import torch

        from . import engine

        if group is not None:
            raise NotImplementedError("mtf() of a sharded frame (group=) is not supported yet")
        nu, theta, planes = _mtf_sampling(frequencies, azimuths, focus)
        axes = pupil_axes(axis, basis)
        _check_reference_name(reference)
        surface_id, generation, n_groups = self._image_selection("mtf", surface, generation, rays_per_source, n_groups,
                                                                 weights)
        rows = self._contiguous_rows()
        dev = rows.device
        centres = None if isinstance(reference, str) else _group_points(reference, n_groups, dev, "reference: a point")
        n_rows = rows.shape[1]
        otf = torch.empty((n_groups, len(planes), len(theta), len(nu), 2), dtype=torch.float64, device=dev)
        record = torch.empty((n_groups, 6), dtype=torch.float64, device=dev)
        engine.call("prt_frame_mtf", *_row_head(rows), *_row_filter(surface_id, generation, rays_per_source, n_groups),
                    centres, axes, _weight_column(weights), nu, len(nu), theta, len(theta), planes, len(planes), otf, record,
                    device=dev, size=(n_rows, n_groups, len(nu), len(theta), len(planes)))
        return MTF(engine.host_complex(otf), engine.host(record), nu, theta, planes)

    # --- geometric encircled / ensquared energy through focus (no counterpart upstream) -------------------------------
    def enclosed_energy(self, surface, radii=None, *, fractions=(0.5, 0.8, 0.9), shape="circle", focus=(0.0,),
                        reference="centroid", follow_centroid=True, axis=None, basis=None, weights="intensity",
                        generation=None, rays_per_source=None, n_groups=None, group=None):
        """The geometric enclosed energy at ``surface`` (an id or an object with ``get_id()``; None: every row that
        passes ``generation``), per group (``id // rays_per_source``) and focus shift: the fraction of the energy within
        each of ``radii`` and, the other way round, the radius that holds each of ``fractions``.  Returns an
        ``EnclosedEnergy``.

        Rays, groups, axes, weights, the centre C_g (``reference``) and each ray's position x(delta) = p + delta s at
        the plane shifted by delta are ``mtf``'s.  Distances are measured from the plane's own weighted centroid
        (``follow_centroid``, the default) or from C_g.  shape: "circle" (sqrt(x1^2 + x2^2)), "square" (max(|x1|, |x2|),
        a half-width), "slit_e2" (|x1|: a slit along e2) or "slit_e1" (|x2|).  radii: None or 1 to 4096 values, finite,
        >= 0 and strictly ascending; fractions: None or 1 to 16 values in (0, 1]; not both None; focus: 1 to 256 shifts.
        The weights are scaled by a power of two to integers, so every sum is exact: the energy is an exact count and
        the radius is the distance of the ray at which the count reaches ceil(fraction * total) -- a ray's own
        distance, not an interpolation (include/prt.h states the definitions).  A weight below 2^-41 of the largest
        (at 1M rays) counts nothing.

        One HIP pass (``prt_frame_energy``) over the rows it selects: frames made by ``where``, ``select`` or under
        ``record_only`` work and give the same bits as the whole frame.  ``group=`` (sharded frames) is not supported
        yet."""
        import torch

        from . import engine

        if group is not None:
            raise NotImplementedError("enclosed_energy() of a sharded frame (group=) is not supported yet")
        edges = np.zeros(0) if radii is None else _mtf_values(radii, "radii", 4096, "finite, >= 0 and strictly ascending",
                                                              non_negative=True)
        if len(edges) > 1 and not np.all(np.diff(edges) > 0):
            raise ValueError("radii: 1 to 4096 numbers, finite, >= 0 and strictly ascending")
        phi = np.zeros(0) if fractions is None else _mtf_values(fractions, "fractions", 16, "in (0, 1]")
        if np.any(phi <= 0) or np.any(phi > 1):
            raise ValueError("fractions: 1 to 16 numbers, in (0, 1]")
        if not len(edges) and not len(phi):
            raise ValueError("radii: give radii, fractions or both")
        if not isinstance(shape, str) or shape not in _ENERGY_SHAPES:
            raise ValueError(f"shape: one of {sorted(_ENERGY_SHAPES)} (got {shape!r})")
        planes = _mtf_values(focus, "focus", 256, "finite shifts along the axis")
        axes = pupil_axes(axis, basis)
        _check_reference_name(reference)
        surface_id, generation, n_groups = self._image_selection("enclosed_energy", surface, generation, rays_per_source,
                                                                 n_groups, weights)
        rows = self._contiguous_rows()
        dev = rows.device
        centres = None if isinstance(reference, str) else _group_points(reference, n_groups, dev, "reference: a point")
        n_rows = rows.shape[1]
        energy = torch.empty((n_groups, len(planes), len(edges)), dtype=torch.float64, device=dev)
        radius = torch.empty((n_groups, len(planes), len(phi)), dtype=torch.float64, device=dev)
        record = torch.empty((n_groups, 10), dtype=torch.float64, device=dev)
        # (radii or fractions that were not asked for are NULL, and so is the output that would hold them: it is empty)
        engine.call("prt_frame_energy", *_row_head(rows), *_row_filter(surface_id, generation, rays_per_source, n_groups),
                    centres, axes, _weight_column(weights), _ENERGY_SHAPES[shape], 1 if follow_centroid else 0,
                    edges if len(edges) else None, len(edges), phi if len(phi) else None, len(phi), planes, len(planes),
                    energy, radius, record, device=dev, size=(n_rows, n_groups, len(edges), len(phi), len(planes)))
        return EnclosedEnergy(engine.host(energy), engine.host(radius), engine.host(record), edges, phi, planes, shape)

    # --- ray-aberration curves: the frame joined by ray id (examples/lens_design.ipynb cells 12-13) ---------------------
    def launch_index(self):
        """Per row, the row number of the generation-0 row with the same ray id (-1: none; a generation-0 row maps to
        itself): a device tensor of ``len(self)`` int64 (``prt_frame_launch_index``: generation 0 writes a dense per-id
        table, every row gathers from it).  It is the notebook's join of two cuts of the frame,
        ``results.loc[(generation == 0) & id.isin(selected.id)]``, as an index.  Ids must be integers, unique within
        generation 0.  Needs the whole frame of a trace, like ``optical_path``."""
        self._need_whole("launch_index", _JOIN_COLUMNS)
        return self._launch_index()

    def _launch_index(self):
        import torch

        from . import engine

        rows = self._contiguous_rows()
        dev = rows.device
        index = torch.empty(rows.shape[1], dtype=torch.int64, device=dev)
        if rows.shape[1] == 0:
            return index
        id0, n_ids, _ = self._id_range("launch_index", rows)
        engine.call("prt_frame_launch_index", *_row_head(rows), int(self.rows_per_generation[0]), id0, n_ids, index,
                    device=dev)
        return index

    def _selection(self, surface, generation):
        """The mask of the rows at ``surface`` (None: any) in ``generation`` (None: any; "last": the highest)."""
        if generation == "last":
            generation = self.last_generation_number() or 0
        mask = None
        if surface is not None:
            mask = self["surface"] == float(surface.get_id() if hasattr(surface, "get_id") else surface)
        if generation is not None:
            m = self["generation"] == float(generation)
            mask = m if mask is None else (mask & m)
        return mask

    def launch(self, surface=None, generation=None):
        """The launch rows of the selected rows (at ``surface``, in ``generation``; "last": the highest), in the
        selected rows' order: a ``DeviceFrame`` aligned row for row with ``where(...)`` of the same selection, without
        the rows that have no launch row.  The notebook's ``results.loc[(generation == 0) & id.isin(selected.id)]``."""
        index = self.launch_index()
        mask = self._selection(surface, generation)
        if mask is not None:
            index = index[mask]
        part = DeviceFrame(self.rows[:, index[index >= 0]], None, self.written)
        part.origin = "launch"
        return part

    def ray_aberrations(self, surface, *, pupil="position", launch_origin=(0.0, 0.0, 0.0), reference="centroid",
                        axis=None, basis=None, pupil_radius=None, zernike=21, zones=64, weights=None, generation=None,
                        rays_per_source=None, n_groups=None, group=None):
        """The ray aberrations at ``surface`` (an id or an object with ``get_id()``; None: every row that passes
        ``generation``) against the pupil coordinate each ray was launched at, per group (``id // rays_per_source``).
        Returns a ``RayAberrations``.

        Every selected row is joined by ray id with its generation-0 row (``launch_index``).  pupil: "position" for
        collimated sources -- h = ((L - O).e1, (L - O).e2), L the launch row's start point, O ``launch_origin`` -- or
        "direction" for point sources -- h = (v.e1, v.e2) / (v.a), v the launch direction.  p = h / rho with rho
        ``pupil_radius`` (None: the group's largest |h|).  Per ray: p, the transverse aberration eps = (Q - C) in
        (e1, e2) about C (``reference``: "centroid" -- the weighted centroid of the group's end points Q --, "chief"
        -- the Q of the ray with the smallest |h| --, a point or an (n_groups, 3) array), the slope
        s = (u.e1, u.e2) / (u.a), and the longitudinal aberration ``axis_intercept`` of the row.  At a plane shifted by
        delta along the axis the transverse aberration is eps + delta s: a through-focus study needs no re-trace.
        ``zernike``: J <= 36 Noll terms fitted to eps1, eps2, s1, s2 over p; ``zones``: 0..1024 rings of equal width in
        |p| for the longitudinal curve; axis / basis / weights as in ``mtf`` (include/prt.h states the definitions).
        Rays without a launch row, with a value that is not finite, with a direction perpendicular to the axis or a
        weight that is not finite and >= 0 count in ``n_missed``.  One HIP pass (``prt_frame_ray_aberrations``), no
        floating-point atomics: the same bits on every run.  Needs the whole frame of a trace, like ``optical_path``;
        ``group=`` (sharded frames) is not supported yet."""
        import torch

        from . import engine

        if group is not None:
            raise NotImplementedError("ray_aberrations() of a sharded frame (group=) is not supported yet")
        if pupil not in ("position", "direction"):
            raise ValueError(f'pupil: "position" or "direction" (got {pupil!r})')
        terms = zernike
        if isinstance(terms, bool) or not isinstance(terms, (int, np.integer)) or not 1 <= terms <= 36:
            raise ValueError(f"zernike: the number of terms, 1 to 36 (got {zernike!r})")
        if isinstance(zones, bool) or not isinstance(zones, (int, np.integer)) or not 0 <= zones <= 1024:
            raise ValueError(f"zones: the number of rings, 0 to 1024 (got {zones!r})")
        terms, zones = int(terms), int(zones)
        if pupil_radius is not None and not (np.isfinite(pupil_radius) and pupil_radius > 0):
            raise ValueError("pupil_radius: a positive number, or None for the group's largest extent")
        origin = np.ascontiguousarray(np.asarray(launch_origin, dtype=np.float64))
        if origin.shape != (3,) or not np.all(np.isfinite(origin)):
            raise ValueError(f"launch_origin: a finite 3-vector (got {launch_origin!r})")
        axes = pupil_axes(axis, basis)
        if isinstance(reference, str) and reference not in ("centroid", "chief"):
            raise ValueError('reference: "centroid", "chief", a point or an (n_groups, 3) array')
        surface_id, generation, n_groups = self._image_selection("ray_aberrations", surface, generation, rays_per_source,
                                                                 n_groups, weights, whole=_JOIN_COLUMNS)
        rows = self._contiguous_rows()
        dev = rows.device
        mode = {"centroid": 0, "chief": 2}.get(reference if isinstance(reference, str) else None, 1)
        centres = None if isinstance(reference, str) else _group_points(reference, n_groups, dev, "reference: a point")
        index = self._launch_index()
        n_rows = rows.shape[1]
        if generation is not None:  # (generation-major: at most one generation's rows are selected)
            capacity = self._generation_slice(generation)[2] if int(generation) >= 0 else 0
        elif surface_id is not None:
            capacity = int((rows[_INDEX["surface"]] == surface_id).sum())
        else:
            capacity = n_rows
        entries = terms * (terms + 1) // 2 + 4 * terms + 1
        rays = torch.empty((capacity, 7), dtype=torch.float64, device=dev)
        row_numbers = torch.empty(capacity, dtype=torch.int64, device=dev)
        record = torch.empty((n_groups, 16), dtype=torch.float64, device=dev)
        normal = torch.empty((n_groups, entries), dtype=torch.float64, device=dev)
        zone = torch.empty((n_groups, zones, 6), dtype=torch.float64, device=dev)
        engine.call("prt_frame_ray_aberrations", *_row_head(rows), index,
                    *_row_filter(surface_id, generation, rays_per_source, n_groups), centres, mode, axes,
                    0 if pupil == "position" else 1, origin, float(pupil_radius or 0.0), terms, zones,
                    _weight_column(weights), capacity, rays, row_numbers, record, normal, zone, device=dev,
                    size=(capacity, n_groups, terms, zones))
        record_host = engine.host(record)
        used = int(record_host[:, 4].sum())
        row_numbers = row_numbers[:used]
        # the launch coordinate itself, gathered from the launch rows (p * rho would round twice)
        launch = rows[:, index[row_numbers]]
        if pupil == "position":
            d = [launch[_INDEX[name]] - float(o) for name, o in zip(("x0", "y0", "z0"), origin)]
            h = [d[0] * float(e[0]) + d[1] * float(e[1]) + d[2] * float(e[2]) for e in (axes[3:6], axes[6:9])]
        else:
            v = [launch[_INDEX[name]] for name in ("x_tilt", "y_tilt", "z_tilt")]
            va = v[0] * float(axes[0]) + v[1] * float(axes[1]) + v[2] * float(axes[2])
            h = [(v[0] * float(e[0]) + v[1] * float(e[1]) + v[2] * float(e[2])) / va for e in (axes[3:6], axes[6:9])]
        groups = None
        if rays_per_source:
            groups = torch.floor(rows[_INDEX["id"]][row_numbers] / float(rays_per_source)).to(torch.int64)
        return RayAberrations(rays[:used], row_numbers, record_host, engine.host(normal), engine.host(zone), terms,
                              h=torch.stack(h, 1), group=groups)

    # --- ray paths: which surfaces every ray met, in order (the frame joined by ray id, for every ray at once) -----------
    def paths(self, weights="intensity", rays_per_source=None, n_groups=None, max_paths=4096):
        """The ray paths of the frame: every ray's ordered sequence of surfaces -- on the host,
        ``results.groupby("id")["surface"].agg(tuple)`` -- put into a tree of prefixes.  Returns a ``Paths``: per node
        (a distinct non-empty prefix of some ray's path) its parent, surface, depth and subtree size, per group
        (``id // rays_per_source``) and node the rays and the energy that went through it, ended there and were
        absorbed there, and per row and per ray the number of its node, so that the frame can be cut by path
        (``frame.select(paths.rows(node))``) and handed to the other passes.

        Nodes are numbered in ascending order of their sequences compared as tuples (``sorted(set(prefixes))``): a
        node's subtree is the range ``[k, k + subtree_size[k])``.  through: the rows at the node; ended: the rays whose
        last row is there; dark: the ended rays whose last row has a direction of length <= 1e-8 (absorbed, as
        ``_pyrayt.py:415`` decides it).  weights: a column name or None for ones; a weight that is not finite and >= 0
        counts 0 (``n_bad_weight``).  The weights are scaled by a power of two to integers, as ``enclosed_energy``
        does, so every sum is exact and the same bits on every run and in any order of the rows of a generation
        (include/prt.h states the definitions).  More than ``max_paths`` (1 to 65536) distinct nodes: ``ValueError``.

        One HIP launch per generation (``prt_frame_paths``).  Ids must be integers, unique within a generation, and
        surfaces integers in [0, 2^31).  Needs the whole frame of a trace, like ``optical_path``."""
        import torch

        from . import engine

        _check_weights(weights)
        if isinstance(max_paths, bool) or not isinstance(max_paths, (int, np.integer)) or not 1 <= max_paths <= 65536:
            raise ValueError(f"max_paths: the most nodes the tree may have, 1 to 65536 (got {max_paths!r})")
        columns = [name for name in _PATHS_COLUMNS if name != "intensity" or weights == "intensity"]
        columns += [weights] if weights is not None and weights not in columns else []
        try:
            self._need_whole("paths", columns=columns)
        except KeyError as error:
            raise ValueError(f"paths: {error.args[0]}") from None
        rows = self._contiguous_rows()
        dev = rows.device
        n_rows = rows.shape[1]
        ids = rows[_INDEX["id"]]
        id0, n_ids, top = self._id_range("paths", rows)
        if rays_per_source:
            if n_groups is None:
                n_groups = max(1, int(top // rays_per_source) + 1)
        else:
            n_groups = 1
        n_groups, max_paths = int(n_groups), int(max_paths)
        row_node = torch.empty(n_rows, dtype=torch.int32, device=dev)
        ray_node = torch.empty(n_ids, dtype=torch.int32, device=dev)
        ray_last_row = torch.empty(n_ids, dtype=torch.int64, device=dev)
        node = torch.empty((max_paths, 4), dtype=torch.int32, device=dev)
        count = torch.empty((n_groups, max_paths, 3), dtype=torch.int64, device=dev)
        energy = torch.empty((n_groups, max_paths, 2), dtype=torch.float64, device=dev)
        record = np.zeros(4, dtype=np.int64)
        counts = np.ascontiguousarray(self.rows_per_generation, dtype=np.int64)
        engine.call("prt_frame_paths", *_row_head(rows)[:3], counts, len(counts), id0, n_ids, float(rays_per_source or 0),
                    n_groups, _weight_column(weights), max_paths, row_node, ray_node, ray_last_row, node, count, energy,
                    record, device=dev, size=(n_rows, n_ids, n_groups, max_paths))
        n_nodes = int(record[0])
        node_host = engine.host(node[:n_nodes])
        count_host = engine.host(count[:, :n_nodes].contiguous())
        energy_host = engine.host(energy[:, :n_nodes].contiguous())
        return Paths(node_host[:, 0], node_host[:, 1], node_host[:, 2], node_host[:, 3], count_host[:, :, 0],
                     count_host[:, :, 1], count_host[:, :, 2], energy_host[:, :, 0], energy_host[:, :, 1],
                     row_node=row_node, ray_node=ray_node, ray_last_row=ray_last_row, id0=id0,
                     n_bad_weight=int(record[2]), n_rays=int(record[1]), ids=ids)

    def fresnel(self, polarization=None, lossless=(), fields=False, coatings=None):
        """Fresnel transmittance and polarisation of every ray, joined by ray id on the device: a ``Fresnel`` with per row
        the share ``transmittance`` of the ray's launch energy that is left when it runs that row's segment -- after
        every interface before it -- and, with ``fields``, the two field vectors carried there.

        An interface is read off two consecutive rows of a ray: the directions and indices before and after, and the
        surface of the earlier row; the normal follows from the two directions.  Unequal indices are a refraction with
        the power-normalised coefficients ts, tp of an uncoated surface; equal indices with a deviated ray are an ideal
        reflection (rs = -1, rp = +1: mirrors, and total internal reflection as the engine writes it; its retardance is
        not modelled); an undeviated ray passes as it is.  ``lossless``: surfaces (ids or objects with ``get_id()`` /
        ``surface_ids``, at most 64 ids) taken as ideally coated: the field is still rotated, with coefficients of
        magnitude 1.  ``polarization``: None for unpolarised input (two orthogonal fields per ray, T their mean), or a
        world vector: each ray starts with its component perpendicular to the launch direction, normalised.  An
        interface the rows cannot describe (a direction or index that is not finite, a transmitted ray on the wrong side)
        makes the ray NaN from there on and counts in ``n_invalid``.  include/prt.h states the definitions.

        ``coatings``: a mapping from a surface (an id, or an object with ``get_id()`` / ``surface_ids``) to a
        ``pyrayt_amd.materials.Coating``: a thin-film stack, a metal (a complex substrate) or a bare face whose total
        internal reflection keeps its phase.  At such a surface the complex amplitude coefficients of the stack replace
        the rules above (characteristic matrices, include/prt.h), the fields are complex and T is computed from them.
        The materials are evaluated on the distinct wavelengths of the frame, at most 256: a continuous Monte-Carlo
        spectrum is out of scope.  At most 64 coated surface ids, 16 coatings of 16 layers.  ``polarization`` may then be
        a complex vector, ``(0, 1, 1j)`` for circular input.  With ``coatings=None`` and a real ``polarization`` the call
        is the one described above, unchanged; otherwise ``field`` is a (6, n) complex128 tensor, the surfaces without
        a coating follow the rules above with the same arithmetic, and the result counts ``n_coated`` and ``n_tir``.

        One HIP launch per generation (``prt_frame_fresnel``, ``prt_frame_fresnel_coated``).  Ids must be integers,
        unique within a generation.  Needs the whole frame of a trace, like ``optical_path``."""
        import torch

        from . import engine

        complex_input = False
        if polarization is not None:
            try:
                complex_input = bool(np.iscomplexobj(np.asarray(polarization)))
            except (TypeError, ValueError):
                complex_input = False
        # the field type: complex (twelve planes, six counters, the coated entry) or real (six planes, four counters)
        is_complex = coatings is not None or complex_input
        try:
            self._need_whole("fresnel", columns=_FRESNEL_COATED_COLUMNS if coatings else _FRESNEL_COLUMNS)
        except KeyError as error:
            raise ValueError(f"fresnel: {error.args[0]}") from None
        ids_lossless = sorted(_lossless_ids(lossless))
        if len(ids_lossless) > 64:
            raise ValueError(f"fresnel: at most 64 lossless surfaces (got {len(ids_lossless)})")
        if is_complex:
            stacks, surface_coating = _coating_stacks(coatings or {}, ids_lossless)
        v = None
        if polarization is not None:
            try:
                v = np.ascontiguousarray(polarization, dtype=np.complex128 if is_complex else np.float64).reshape(-1)
            except (TypeError, ValueError):
                v = np.zeros(0)
            if v.shape != (3,) or not np.all(np.isfinite(v)) or not np.any(v != 0):
                raise ValueError("fresnel: polarization is None or a world vector of three finite numbers, not all zero")
        rows = self._contiguous_rows()
        dev = rows.device
        n_rows = rows.shape[1]
        id0, n_ids, _ = self._id_range("fresnel", rows)
        entry, tables, planes, counters = "prt_frame_fresnel", (), 6, 4
        if is_complex:
            entry, planes, counters = "prt_frame_fresnel_coated", 12, 6
            tables = _coating_tables(stacks, surface_coating, rows if n_rows else None)
        transmittance = torch.empty(n_rows, dtype=torch.float64, device=dev)
        field = torch.empty((planes, n_rows), dtype=torch.float64, device=dev) if fields else None
        record = np.zeros(counters, dtype=np.int64)
        counts = np.ascontiguousarray(self.rows_per_generation, dtype=np.int64)
        lossless_ids = np.ascontiguousarray(ids_lossless, dtype=np.int64)
        parts = None if v is None else np.ascontiguousarray(np.concatenate([v.real, v.imag]) if is_complex else v)
        engine.call(entry, *_row_head(rows)[:3], counts, len(counts), id0, n_ids, parts,
                    lossless_ids if len(lossless_ids) else None, len(lossless_ids), *tables, transmittance, field, record,
                    device=dev, size=(n_rows, n_ids))
        if not is_complex:
            out = Fresnel(self, transmittance, field, record, polarization=v, lossless=tuple(ids_lossless))
        else:
            field = torch.complex(field[:6], field[6:]) if field is not None else None
            out = Fresnel(self, transmittance, field, record, polarization=v, lossless=tuple(ids_lossless),
                          coatings=dict(coatings or {}))
        out.launch_states = "per_ray" if v is None else "polarised"
        return out

    def ghosts(self, fresnel, surfaces=None, rays_per_source=None, n_groups=None, min_intensity=0.0, ray_offset=1e-6,
               system=None):
        """The ghost rays of the frame: at every refraction the rows describe, at ``surfaces``, one reflected child ray
        with the energy ``fresnel`` (``self.fresnel(...)``, of this very frame) says did not go through,
        ``intensity[p] * (T[p] - T[j])`` for a ray's consecutive rows p, j.  Returns a ``pyrayt_amd.ghosts.GhostRays``:
        the (13, n) ray set, ordered by (parent group, surface) so that every ghost path is a source of the per-source
        passes of its trace, per child the row it left, the groups' keys and the counters.  ``surfaces``: ids, objects
        with ``get_id()`` or components, at most 64 ids; None: every refracting surface of ``system`` (components, a
        tracer or a snapshot).  ``rays_per_source`` / ``n_groups``: the parent groups, ``id // rays_per_source`` (at
        most 65535 groups x surfaces).  ``min_intensity``: children below it are dropped and counted.  ``ray_offset``:
        how far a child starts off its surface.  A ray that leaves the system has no later row, so the reflection at
        the end of its last row is not seen: ``n_open`` counts such rows (``pyrayt_amd.ghosts.housing``).  Refused: a
        frame that is not whole, a ``Fresnel`` of another frame, coatings with an absorbing layer at a listed
        surface (there R is not 1 - T).  One HIP launch per generation and the image passes' stable counting sort;
        include/prt.h states the definitions."""
        from . import ghosts

        return ghosts.spawn(self, fresnel, surfaces, rays_per_source, n_groups, min_intensity, ray_offset, system)

    def scatter(self, models, system, toward=None, rays_per_hit=1, seed=0, rays_per_source=None, n_groups=None,
                min_intensity=0.0, ray_offset=1e-6):
        """The scattered rays of the frame: every row that lands on a surface of ``models`` -- a dict ``{surface |
        component | tuple of them: pyrayt_amd.scatter.Scatter}``, at most 64 surfaces and 16 models -- sends
        ``rays_per_hit`` (1 to 64) child rays back into the half space it came from, whatever happens to its ray
        afterwards.  ``toward=None`` draws them cosine-weighted over the hemisphere, ``E = 4 I f / N`` each;
        ``toward=Target.disk(centre, normal, radius)`` sends them to uniform points of the disk, ``E = I f cos_o cos_t
        4 R^2 / (N r^2)``: importance sampling towards an imager.  ``system`` (components, a tracer or a snapshot)
        gives the primitive behind every surface id and so the normal.  Random numbers are Philox4x32-10 on (``seed``,
        ray id, generation, child): a child does not depend on where its row stands or on the other rows.  Returns a
        ``pyrayt_amd.scatter.ScatterRays``, the interface of ``GhostRays``: the (13, n) ray set ordered by (source,
        surface) with the children of a bucket in (row, child) order, ``parent_row``, ``child``, the groups' keys and
        the counters.  To scatter what is left after Fresnel losses call it on ``fresnel.apply()``.  The frame need not
        be whole.  One HIP pass and the image passes' stable counting sort; include/prt.h states the definitions."""
        from . import scatter

        return scatter.spawn(self, models, system, toward, rays_per_hit, seed, rays_per_source, n_groups, min_intensity,
                             ray_offset)

    # --- sensitivities: differential ray tracing (no counterpart upstream) -------------------------------------------
    def sensitivity(self, surface, parameters, system, *, weights="intensity", reference="centroid", generation=None,
                    rays_per_source=None, n_groups=None, wavefront=None, slopes=False):
        """d(landing point)/d(parameter) at ``surface`` for motions, shape changes and index changes of parts, and for
        motions of the rays' launch and changes of their wavelength, from this one trace: a ``Sensitivity``.
        ``parameters``: up to 16 of ``Motion`` (a rigid motion), ``Deformation`` (an affine deformation: radii, a
        paraboloid's focus, heights, sides and thicknesses), ``IndexChange`` (the index of a glass), ``SourceMotion`` (a
        rigid motion of the launch of rays: field points, the ray-transfer matrix, focal lengths) and ``WavelengthChange``
        (colour: the Sellmeier glasses' own dispersion), in any mix; a call of Motions alone runs
        ``prt_frame_sensitivity`` as it always did, a call without the last two kinds ``prt_frame_design_sensitivity`` as
        it always did, and a call with one of them ``prt_frame_launch_sensitivity``, in which the other kinds have the
        same bits and which also gives ``slopes``, the derivative of the rows' directions (``focus_gradient``,
        ``transfer``, ``effective_focal_length``).  A ``WavelengthChange`` needs the frame's ``wavelength`` column and
        raises ``ValueError`` for a system with a table glass.  ``system``: the components the frame was
        traced through (or their ``SceneSnapshot``), whose snapshot -- the one the scene compiler takes -- tells the
        pass the kind, parameters and transform of the primitive behind every ``surface`` id.

        A tangent (d position, d direction) per ray and parameter is pushed through the interfaces the ray's rows
        describe, joined by ray id on the device (``prt_frame_sensitivity``; include/prt.h states the formulas): one
        HIP launch per generation, no re-trace.  The rows selected are those that end on ``surface`` (an id or an
        object with ``get_id()``), of every generation or of ``generation`` (a number or "last").  Per group (``id //
        rays_per_source``, as in ``wavefront``) and with ``weights`` (a column, or None for 1) the pass also sums what
        the gradient of the spot size and a least-squares step need.  ``reference``: "centroid", a point or an
        (n_groups, 3) array: what the mean square radius is taken about.

        A ray that meets a surface that is not in ``system``, a row that is not finite, or an interface whose rows fit
        neither Snell's law nor a reflection (a caller-shaded material) is NaN from there on and is counted
        (``n_unknown``, ``n_invalid``, ``n_unfit``); the sums leave such rows out.

        ``wavefront``: a ``Wavefront`` of this frame at the same ``surface``, ``generation``, groups and ``weights``
        (``ValueError`` for any other), or True for ``self.wavefront(surface, ...)`` with its defaults and these.  The
        call then runs ``prt_frame_opd_sensitivity``: the same pass with the derivative of the optical path carried along,
        and the ``Sensitivity`` also has the wavefront change per parameter against that Wavefront's reference sphere,
        HELD FIXED (``dfield``, ``dopd``, ``dpupil``, ``dzernike()``, ``rms_opd_gradient``, ``step(merit="wavefront")``);
        ``jacobian`` and the landing-point sums keep their bits.  Without it nothing changes.

        ``slopes=True``: the call goes through ``prt_frame_launch_sensitivity`` whatever the parameters are (with or
        without ``wavefront=``; a parameter that is neither a ``SourceMotion`` nor a ``WavelengthChange`` has no flags
        there) and the ``Sensitivity`` has ``slopes``, which ``mtf_gradient()`` needs; ``jacobian``, the sums and the
        wavefront outputs keep their bits.  With the default every call takes the entry point it always took.

        Out of scope: a reference radius that changes with the parameter; rays whose path changes under the
        parameter, such as those at the edge of an aperture -- the result is the derivative at fixed path, as in every
        differential ray trace.  Known limits: an interface whose two indices are equal to the bit is differentiated
        as no interface at all, whatever an ``IndexChange`` or a ``WavelengthChange`` says of it; a ray launched inside a
        glass keeps the index of its first segment under a ``WavelengthChange``.
        Needs the whole frame of a trace, like ``optical_path``."""
        import torch

        from . import engine

        motions, form = _sens_parameters(parameters, rays_per_source, slopes)
        _check_weights(weights)
        _check_reference_name(reference)
        if surface is None:
            raise ValueError("sensitivity: surface is an id or an object with get_id()")
        surface_id = float(_surface_id(surface))
        if wavefront is not None and wavefront is not True and not isinstance(wavefront, Wavefront):
            raise ValueError("wavefront: a Wavefront of this frame, True or None")
        snapshot, prims = _sens_primitives(system, motions, form["colour"])
        try:
            self._need_whole("sensitivity", columns=_PATH_COLUMNS + (("wavelength",) if form["colour"] else ())
                             + ((weights,) if weights else ()))
        except KeyError as error:
            raise ValueError(f"sensitivity: {error.args[0]}") from None
        rows = self._contiguous_rows()
        dev = rows.device
        n_rows = rows.shape[1]
        id0, n_ids, top = self._id_range("sensitivity", rows)
        n_groups = int(_group_count(rays_per_source, n_groups, lambda: top))
        if not 1 <= n_groups <= 65535:
            raise ValueError("sensitivity: 1 to 65535 groups")
        K = len(motions)
        counts = np.ascontiguousarray(self.rows_per_generation, dtype=np.int64)
        if generation == "last":
            generation = self.last_generation_number() or 0
        if wavefront is True:
            wavefront = self.wavefront(surface_id, weights=weights, generation=generation,
                                       rays_per_source=rays_per_source, n_groups=n_groups)
        if wavefront is not None:
            made = _sens_made_of(wavefront, dict(
                frame=self, surface=surface_id, generation=None if generation is None else int(generation),
                rays_per_source=float(rays_per_source or 0), n_groups=n_groups, weights=weights))
        # (plumbing with a price: the id range above, group_first and the pivots below are each read back to the host
        # and wait for the stream, before a call that synchronises itself: part of the call's fixed cost, see
        # profiles/sensitivity/README.md)
        selected, row_slot, group_first = _sens_selection(rows, surface_id, generation, rays_per_source, n_groups, id0,
                                                          n_ids, len(counts))
        n_selected = int(selected.shape[0])
        pivots, centred = _sens_pivots(rows, reference, selected, group_first, n_groups)
        # (a call of Motions alone, without slopes=True, takes the entry point, the kernel and the workspace it always took)
        name = ("launch" if form["launch_form"] else "wavefront" if wavefront is not None else "design" if form["design"]
                else "rigid")
        if name == "launch" and wavefront is not None and not n_rows:
            # (the entry point reads opl == NULL as "no wavefront": there is no path to point at)
            raise ValueError("sensitivity: wavefront= with a SourceMotion, a WavelengthChange or slopes=True needs a frame with rows")
        size_extra, entry, order = _SENS_FORMS[name]
        empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
        jacobian, sums = empty(K, 3, n_selected), empty(n_groups, 6 + 4 * K + K * (K + 1) // 2)
        directions = empty(K, 3, n_selected) if name == "launch" else None
        record = np.zeros(4, dtype=np.int64)
        pieces = dict.fromkeys(_SENS_WAVE_IN + _SENS_WAVE_OUT)  # (the launch form without wavefront= passes these as NULL)
        device, _, ld, _ = _row_head(rows)
        pieces.update(_sens_host_arrays(motions, name, snapshot.materials), n_terms=0,
                      device=device, rows=rows, ld=ld, counts=counts, n_generations=len(counts),
                      id0=id0, n_ids=n_ids, prims=prims, n_prims=len(prims), K=K,
                      row_slot=row_slot, selected=selected, n_selected=n_selected, group_first=group_first,
                      n_groups=n_groups, weight_column=_weight_column(weights), pivots=pivots,
                      jacobian=jacobian, sums=sums, slopes=directions, record=record)
        wave = None
        if wavefront is not None:
            J = wavefront.terms
            wave = dict(dfield=empty(K, n_selected), dopd=empty(K, n_selected), dpupil=empty(K, 2, n_selected),
                        opd=empty(n_selected), pupil=empty(n_selected, 2),
                        sums=empty(n_groups, 5 + J * (K + 3) + 4 * K + K * (K + 1) // 2))
            pieces.update({q: wave[q] for q in _SENS_WAVE_OUT[:-1]}, opd_sums=wave["sums"], n_terms=J,
                          opl=self._optical_path(),
                          groups=np.ascontiguousarray(np.column_stack([wavefront.reference, wavefront.radius,
                                                                       wavefront.pivot, wavefront.pupil_radius]),
                                                      dtype=np.float64),
                          axes=np.ascontiguousarray(made["axes"], dtype=np.float64))
        engine.call(entry, *(pieces[q] for q in order), device=dev, size=(
            n_ids, len(prims), K, n_groups, int(np.diff(group_first).max()), *(pieces[q] for q in size_extra)))
        if wave is not None:
            wave.update(sums=engine.host(wave["sums"]), wavefront=wavefront)
        launch = None
        if name in ("wavefront", "launch"):
            launch = dict(slopes=directions, rows=rows, weights=weights, group_first=group_first, written=self.written)
        return Sensitivity(jacobian, selected, engine.host(sums), pivots, centred, record, motions, wave=wave, launch=launch)

    def axis_intercept(self):
        """x where each ray's line crosses the optical (x) axis in the xy plane, from the segment's start point as the
        notebook writes it (cells 12, 15): ``x0 - x_tilt * y0 / y_tilt``."""
        return self["x0"] - self["x_tilt"] * self["y0"] / self["y_tilt"]

    def spot(self, plane=("y1", "z1")):
        """(centroid, rms radius) of the end points in a transverse plane."""
        if tuple(plane) == ("y1", "z1") and getattr(self.rows, "is_cuda", False) and len(self):
            stats = self.group_stats().iloc[0]
            return (float(stats["y"]), float(stats["z"])), float(stats["rms_radius"])
        a, b = self[plane[0]], self[plane[1]]
        ca, cb = a.mean(), b.mean()
        rms = (((a - ca) ** 2 + (b - cb) ** 2).mean()) ** 0.5
        return (float(ca), float(cb)), float(rms)

    def axis_crossing(self):
        """x where each ray of this frame crosses the optical (x) axis in the xy plane:
        x1 - y1 * x_tilt / y_tilt (the paraxial-focus estimate of the lens-design notebook)."""
        return self["x1"] - self["y1"] * self["x_tilt"] / self["y_tilt"]

    # --- export -------------------------------------------------------------------------------------
    def to_numpy(self):
        """(R, columns) float64 view of a host copy (one D2H transfer; a frame recorded with a column list brings only
        those columns across)."""
        from . import engine

        if self.written is not None:
            return engine.to_host(self.rows[list(self.written)]).T  # (the written columns gathered on the device first)
        return engine.to_host(self.rows).T  # a strided view crosses PCIe as it is: no device-side repack

    def to_pandas(self):
        values = self.to_numpy()
        if values.shape[0] == 0:
            return pd.DataFrame(columns=self.columns, dtype="float64")
        return pd.DataFrame(values, columns=self.columns, copy=False)


class SinkStats:
    """The sums a trace under a ``RecordPlan(stats=True)`` accumulated in its generation kernels -- per generation and
    per group what ``prt_frame_reduce`` / ``prt_frame_mean_square`` would have read back out of the stored frame --
    turned into the tables ``DeviceFrame.group_stats`` / ``mean_square`` return.  One small device-to-host copy (96
    bytes per generation and group); the frame itself was never written."""

    def __init__(self, sums, pivots=None, about=0.0):
        """sums: (generations, n_groups, 12) tensor or array; pivots: (n_groups, 3) the sums were taken about."""
        host = sums.detach().cpu().numpy() if hasattr(sums, "detach") else np.asarray(sums)
        self.sums = np.array(host, dtype=float)
        piv = None if pivots is None else (pivots.detach().cpu().numpy() if hasattr(pivots, "detach") else np.asarray(pivots))
        self.pivots = np.zeros((self.sums.shape[1], 3)) if piv is None else np.array(piv, dtype=float)

    def last_generation_number(self):
        """The highest generation that counted a row the plan let pass (None: no row passed).  With a surface filter
        this may be lower than the frame's last generation: rays that miss the filtered surfaces can live on."""
        working = np.nonzero(self.sums[:, :, 0].sum(axis=1) > 0)[0]
        return int(working[-1]) if len(working) else None

    def _block(self, generation):
        if generation is None:
            return self.sums.sum(axis=0)   # (additive over generations: one set of pivots)
        if generation == "last":
            generation = self.last_generation_number()
            if generation is None:
                return np.zeros(self.sums.shape[1:])
        if not 0 <= int(generation) < self.sums.shape[0]:
            return np.zeros(self.sums.shape[1:])
        return self.sums[int(generation)]

    def group_stats(self, generation=None):
        """The table of ``DeviceFrame.group_stats`` (count, y, z, rms_radius, focus, focus_std, wavelength, intensity per
        source) for the rows the plan let pass, of one generation (a number, or "last": the highest that counted a
        row the plan let pass -- not necessarily the frame's last generation) or of all of them (None).  Same arithmetic as ``k_frame_finish`` (csrc/prt_frame.hpp)."""
        frame = pd.DataFrame(self.values(generation))
        frame.index.name = "source_id"
        return frame

    def values(self, generation=None):
        """``group_stats`` as a dict of numpy arrays (one entry per source): what a merit function reads in a loop,
        without the 0.2 ms a DataFrame takes to build."""
        s = self._block(generation)
        count, with_focus = s[:, 0], s[:, 8]
        with np.errstate(invalid="ignore", divide="ignore"):
            safe, safe_f = np.where(count > 0, count, 1.0), np.where(with_focus > 0, with_focus, 1.0)
            dy, dz, df = s[:, 1] / safe, s[:, 2] / safe, s[:, 4] / safe_f
            var_r = np.maximum(s[:, 3] / safe - dy * dy - dz * dz, 0.0)
            var_f = np.maximum(s[:, 5] / safe_f - df * df, 0.0)
            nan = np.nan
            return {
                "count": count.astype(np.int64),
                "y": np.where(count > 0, self.pivots[:, 0] + dy, nan), "z": np.where(count > 0, self.pivots[:, 1] + dz, nan),
                "rms_radius": np.where(count > 0, np.sqrt(var_r), nan),
                "focus": np.where(with_focus > 0, self.pivots[:, 2] + df, nan),
                "focus_std": np.where(with_focus > 0, np.sqrt(var_f), nan),
                "wavelength": np.where(count > 0, s[:, 6] / safe, nan), "intensity": np.where(count > 0, s[:, 7] / safe, nan),
            }

    def mean_square(self, generation=None, per_source=False):
        """``np.mean(np.square(f(rows) - about))`` of the plan's ``mean_square`` quantity (``DeviceFrame.mean_square``):
        a float over the rows of every group, or per source a DataFrame (count, mean, mean_square)."""
        s = self._block(generation)
        if not per_source:  # (over the rows of every group, as DeviceFrame.mean_square without rays_per_source)
            count = s[:, 9].sum()
            return float(s[:, 11].sum() / count) if count > 0 else float("nan")
        with np.errstate(invalid="ignore", divide="ignore"):
            mean, mean_square = s[:, 10] / s[:, 9], s[:, 11] / s[:, 9]
        frame = pd.DataFrame({"count": s[:, 9].astype(np.int64), "mean": mean, "mean_square": mean_square})
        frame.index.name = "source_id"
        return frame


_PATH_COLUMNS = ("index", "id", "surface", "generation", "x0", "y0", "z0", "x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")
_JOIN_COLUMNS = tuple(name for name in _PATH_COLUMNS if name != "index")  # (what the ray-aberration passes read)
_MTF_COLUMNS = ("x1", "y1", "z1", "x_tilt", "y_tilt", "z_tilt")  # (what the MTF reads of every ray)
_PATHS_COLUMNS = ("generation", "intensity", "id", "surface", "x_tilt", "y_tilt", "z_tilt")  # (what paths() reads)
_FRESNEL_COLUMNS = ("generation", "intensity", "index", "id", "surface", "x_tilt", "y_tilt", "z_tilt")  # (fresnel())
_FRESNEL_COATED_COLUMNS = _FRESNEL_COLUMNS + ("wavelength",)  # (fresnel(coatings=...))
_ENERGY_SHAPES = {"circle": 0, "square": 1, "slit_e1": 2, "slit_e2": 3}  # (PRT_ENERGY_* of include/prt.h)


class Wavefront:
    """What ``DeviceFrame.wavefront`` returns.  Per selected row, in row order (device tensors): ``opd`` -- the optical
    path difference against the reference sphere with the group's mean taken off, NaN for a ray that misses the
    sphere -- and ``pupil`` (n, 2), the normalised pupil point (e1, e2), ``theta = atan2(pupil[:, 1], pupil[:, 0])``.
    Per group (numpy arrays): ``rms`` and ``pv`` of the OPD, ``zernike`` (n_groups, J) -- Noll's Z1..ZJ; Z1 is the piston
    about the pivot --, ``rank`` of the fit's normal equations, ``n_rays`` (rows that met the sphere), ``n_missed``;
    ``reference`` (P), ``radius`` (R), ``pivot``, ``pupil_radius``; ``normal``: the device's sums (the upper triangle
    of Z^T W Z by rows, Z^T W OPD, sum w, sum w OPD, sum w OPD^2; OPD about the pivot)."""

    def __init__(self, opd, pupil, record, normal, terms):
        self.opd, self.pupil, self.normal, self.terms = opd, pupil, normal, terms
        self.reference, self.radius, self.pivot = record[:, 0:3], record[:, 3], record[:, 4]
        self.pupil_radius = record[:, 5]
        rows, self.n_missed = record[:, 6].astype(np.int64), record[:, 7].astype(np.int64)
        self.n_rays = rows - self.n_missed
        self.pv = record[:, 8] - record[:, 9]
        self.zernike, self.rank = solve_normal_equations(normal, terms)
        w, wv, wvv = normal[:, -3], normal[:, -2], normal[:, -1]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = wv / w
            self.rms = np.where(w > 0, np.sqrt(np.maximum(wvv / w - mean * mean, 0.0)), np.nan)

    def to_pandas(self):
        """One row per group: n_rays, n_missed, rms, pv, rank, Z1..ZJ."""
        frame = pd.DataFrame({"n_rays": self.n_rays, "n_missed": self.n_missed, "rms": self.rms, "pv": self.pv,
                              "rank": self.rank})
        for j in range(self.terms):
            frame[f"Z{j + 1}"] = self.zernike[:, j]
        frame.index.name = "source_id"
        return frame


class PSF:
    """What ``DeviceFrame.psf`` returns (numpy arrays).  ``image`` (n_groups, nx, ny): the normalised polychromatic
    image, indexed (e1, e2) as ``np.histogram2d`` is (``imshow(image[g].T, origin="lower")`` is upright);
    ``image_by_wavelength`` (n_groups, n_wavelengths, nx, ny), whose sum over wavelengths is ``image``; ``u`` (nx) and
    ``v`` (ny): the pixel centres along e1 and e2, in world units, about P; per group ``strehl`` (the image at P),
    ``peak`` and ``peak_uv`` (the brightest pixel and its centre), ``f_number`` (R / (2 rho_max)), ``n_rays`` (rays
    summed) and ``n_missed`` (rays left out: they missed the reference sphere or had no usable weight);
    ``wavelengths`` (micrometres); ``record`` (n_groups, n_wavelengths, 4): rays used, rays left out, sum of the
    amplitudes, Strehl numerator; ``wavefront``: the ``Wavefront`` the image was built on."""

    def __init__(self, image_by_wavelength, strehl, record, wavelengths, world_unit_um, pixels, pixel_size, centre,
                 f_number, wavefront):
        self.image_by_wavelength = image_by_wavelength
        self.image = image_by_wavelength.sum(axis=1)
        self.strehl, self.record, self.wavelengths = strehl, record, np.asarray(wavelengths, dtype=float)
        self.world_unit_um, self.pixel_size, self.centre = world_unit_um, pixel_size, centre
        self.f_number, self.wavefront = f_number, wavefront
        nx, ny = pixels
        self.u = centre[0] + (np.arange(nx) - 0.5 * (nx - 1)) * pixel_size[0]
        self.v = centre[1] + (np.arange(ny) - 0.5 * (ny - 1)) * pixel_size[1]
        self.n_rays = record[:, :, 0].sum(axis=1).astype(np.int64)
        self.n_missed = record[:, :, 1].sum(axis=1).astype(np.int64)
        flat = self.image.reshape(len(self.image), -1)
        self.peak = np.full(len(flat), np.nan)
        self.peak_uv = np.full((len(flat), 2), np.nan)
        for g, values in enumerate(flat):
            if np.all(np.isfinite(values)):
                i, j = np.unravel_index(int(np.argmax(values)), (nx, ny))
                self.peak[g], self.peak_uv[g] = values[i * ny + j], (self.u[i], self.v[j])

    def encircled_energy(self, radii, about="reference"):
        """Per group, the share of the window's total in the pixels whose centres lie within each radius (world units)
        of P (``about="reference"``) or of the brightest pixel (``"peak"``): an array (n_groups, len(radii)), or
        (n_groups,) for one radius.  A host-side sum on the image: the window must hold what is to be counted."""
        if about not in ("reference", "peak"):
            raise ValueError('about: "reference" or "peak"')
        r = np.atleast_1d(np.asarray(radii, dtype=float))
        out = np.full((len(self.image), len(r)), np.nan)
        for g, image in enumerate(self.image):
            cu, cv = (0.0, 0.0) if about == "reference" else self.peak_uv[g]
            dist = np.hypot(self.u[:, None] - cu, self.v[None, :] - cv)
            total = image.sum()
            out[g] = [image[dist <= radius].sum() / total for radius in r]
        return out[:, 0] if np.ndim(radii) == 0 else out

    def to_pandas(self):
        """One row per group: strehl, peak, peak_u, peak_v, f_number, n_rays, n_missed."""
        frame = pd.DataFrame({"strehl": self.strehl, "peak": self.peak, "peak_u": self.peak_uv[:, 0],
                              "peak_v": self.peak_uv[:, 1], "f_number": self.f_number, "n_rays": self.n_rays,
                              "n_missed": self.n_missed})
        frame.index.name = "source_id"
        return frame

    def mtf(self, frequencies, azimuths=(0.0, 90.0)):
        """The MTF of this image (the Huygens MTF, for systems near the diffraction limit where the geometric MTF does
        not apply): per group the DFT of ``image`` at k = nu (cos theta, sin theta), normalised by the image's sum, with
        the pixel centres (u, v) about P as coordinates.  frequencies in cycles per world unit, azimuths in degrees from
        e1 towards e2.  A host-side sum; the window must hold the image.  Returns an ``MTF`` with one focus plane."""
        nu = _mtf_values(frequencies, "frequencies", 4096, "finite and >= 0", non_negative=True)
        theta = _mtf_values(azimuths, "azimuths", 16, "finite, in degrees")
        rad = np.radians(theta)
        kc, ks = np.cos(rad)[:, None] * nu[None, :], np.sin(rad)[:, None] * nu[None, :]
        n = len(self.image)
        otf = np.full((n, 1, len(theta), len(nu)), np.nan, dtype=complex)
        record = np.full((n, 6), np.nan)
        for g, image in enumerate(self.image):
            total = image.sum()
            along_u = np.exp(-2j * np.pi * kc[..., None] * self.u)  # (azimuths, frequencies, nx)
            along_v = np.exp(-2j * np.pi * ks[..., None] * self.v)  # (azimuths, frequencies, ny)
            otf[g, 0] = np.einsum("afi,ij,afj->af", along_u, image, along_v) / total
            record[g, 3:] = total, self.n_rays[g], self.n_missed[g]
        return MTF(otf, record, nu, theta, np.zeros(1))


class PSFScan:
    """What ``DeviceFrame.psf(focus=...)`` returns: the diffraction PSF and the Strehl ratio on F planes shifted along
    the axis, G groups, L wavelengths (numpy arrays unless stated).  ``image_by_wavelength`` (G, F, L, nx, ny) and
    ``image`` (G, F, nx, ny), normalised as ``PSF.image`` is, by the same denominator on every plane; ``strehl`` (G, F):
    the normalised intensity at the chief line's point of plane f, P + delta_f (t1 e1 + t2 e2 + a) -- on the axis line
    with ``track=None`` --, whatever ``centre`` and the grid; ``focus`` (F); ``line`` (G, 2): the chief line's slopes
    (t1, t2), 0 with ``track=None``; ``centres`` (G, F, 2): each grid's centre, (u0 + delta t1, v0 + delta t2); ``u`` (nx)
    and ``v`` (ny): the pixel centres as offsets from a plane's centre; ``record`` (G, L, 4) as ``PSF.record``, the same
    for every plane, and ``n_rays`` / ``n_missed``; ``peak`` (G, F): the brightest pixel; ``wavelengths``, ``f_number``,
    ``wavefront``; ``axial``: a device tensor like ``wavefront.pupil``, per selected row in the wavefront's order the
    component (E - P).a of its point on the reference sphere, NaN where the ray misses it."""

    def __init__(self, image_by_wavelength, strehl, record, axial, line, centres, focus, wavelengths, world_unit_um,
                 pixels, pixel_size, centre, f_number, wavefront, track="chief"):
        self.image_by_wavelength = image_by_wavelength
        self.image = image_by_wavelength.sum(axis=2)
        self.strehl, self.record, self.axial = np.asarray(strehl, dtype=float), record, axial
        self.line, self.centres = np.asarray(line, dtype=float), np.asarray(centres, dtype=float)
        self.focus, self.wavelengths = np.asarray(focus, dtype=float), np.asarray(wavelengths, dtype=float)
        self.world_unit_um, self.pixels, self.pixel_size, self.centre = world_unit_um, pixels, pixel_size, centre
        self.f_number, self.wavefront, self.track = f_number, wavefront, track
        nx, ny = pixels
        self.u = (np.arange(nx) - 0.5 * (nx - 1)) * pixel_size[0]
        self.v = (np.arange(ny) - 0.5 * (ny - 1)) * pixel_size[1]
        self.n_rays = record[:, :, 0].sum(axis=1).astype(np.int64)
        self.n_missed = record[:, :, 1].sum(axis=1).astype(np.int64)
        flat = self.image.reshape(self.image.shape[0], self.image.shape[1], -1)
        with np.errstate(invalid="ignore"):
            self.peak = np.where(np.all(np.isfinite(flat), axis=2), flat.max(axis=2, initial=-np.inf), np.nan)

    def plane(self, delta, group=None):
        """The ``PSF`` of one of ``focus``: its ``encircled_energy()``, ``mtf()`` and ``to_pandas()`` then work on that
        plane, with the pixel centres about the plane's point on the axis line through P.  A ``PSF`` has one grid for
        all its groups: where the groups' centres differ on this plane (tracked chief lines), give ``group`` -- the
        result then holds that group alone."""
        f = _positions(self.focus, [delta], "delta")[0]
        groups = slice(None) if group is None else slice(int(group), int(group) + 1)
        centres = self.centres[groups, f]
        if len(centres) and not np.all((centres == centres[0]) | np.isnan(centres)):
            raise ValueError("plane: the groups' grids have different centres on this plane; give group=")
        finite = centres[np.all(np.isfinite(centres), axis=1)]
        centre = tuple(float(x) for x in finite[0]) if len(finite) else self.centre
        return PSF(self.image_by_wavelength[groups, f], self.strehl[groups, f], self.record[groups], self.wavelengths,
                   self.world_unit_um, self.pixels, self.pixel_size, centre, np.asarray(self.f_number)[groups],
                   self.wavefront)

    def best_focus(self):
        """Per group, the focus shift of the largest Strehl ratio: the best sampled plane, refined by the vertex of the
        parabola through it and its two neighbours when it is not at an end of the scan (``MTF.best_focus``'s rule).
        NaN for a group without rays."""
        return _best_plane(self.focus, self.strehl)

    def to_pandas(self):
        """Long form: one row per (source_id, focus) with its strehl and peak."""
        g, f = self.strehl.shape
        index = np.indices((g, f)).reshape(2, -1)
        return pd.DataFrame({"source_id": index[0], "focus": self.focus[index[1]], "strehl": self.strehl.reshape(-1),
                             "peak": self.peak.reshape(-1)})


class VectorPSF(PSF):
    """What ``DeviceFrame.psf(fresnel=...)`` returns: a ``PSF`` of the polarised Huygens sum (numpy arrays).  ``image``
    and ``image_by_wavelength`` are S0 + axial, the mean over the input states, over the scalar PSF's own denominator
    D_g (the perfect, lossless wave with parallel fields on the same rays).  Besides what a ``PSF`` has:
    ``stokes`` (n_groups, 4, nx, ny) and ``stokes_by_wavelength`` (n_groups, n_wavelengths, 4, nx, ny): S0..S3 of the
    transverse field in (e1, e2), the convention of ``Fresnel.stokes``; ``axial`` (n_groups, nx, ny) and
    ``axial_by_wavelength``: |U3|^2, the field along the axis; per group ``strehl`` (the image at P over D_g: comparable
    with the scalar ``psf()`` of the bare frame and across coatings), ``strehl_apodized`` (the image at P over the same
    amplitudes with phases and field directions aligned: the strict ratio), ``throughput`` (sum w |E|^2 / sum w over
    the rays summed) and ``denominator`` (D_g); ``record`` (n_groups, n_wavelengths, n_states, 6): rays used, rays
    left out, sum sqrt(w), sum |A|, Strehl numerator, sum w |E|^2; ``n_states`` (1: polarised input, 2: unpolarised);
    ``fresnel``: the ``Fresnel`` whose fields were summed."""

    def __init__(self, stokes, strehl, record, wavelengths, world_unit_um, pixels, pixel_size, centre, f_number,
                 wavefront, fresnel=None):
        super().__init__(stokes[:, :, 0] + stokes[:, :, 4], strehl[:, 0], record[:, :, 0, :], wavelengths,
                         world_unit_um, pixels, pixel_size, centre, f_number, wavefront)
        self.record, self.n_states, self.fresnel = record, record.shape[2], fresnel
        self.stokes_by_wavelength, self.axial_by_wavelength = stokes[:, :, :4], stokes[:, :, 4]
        self.stokes, self.axial = self.stokes_by_wavelength.sum(axis=1), self.axial_by_wavelength.sum(axis=1)
        self.strehl_apodized, self.throughput, self.denominator = strehl[:, 1], strehl[:, 2], strehl[:, 3]

    def degree_of_polarization(self):
        """sqrt(S1^2 + S2^2 + S3^2) / S0 per pixel of the polychromatic image, (n_groups, nx, ny); NaN where S0 is 0."""
        s = self.stokes
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sqrt(s[:, 1] ** 2 + s[:, 2] ** 2 + s[:, 3] ** 2) / s[:, 0]

    def analyzed(self, jones):
        """The image behind an ideal analyser that passes the transverse state ``jones`` = (j1, j2) in (e1, e2), complex
        in general ((1, 0): linear along e1; (1, 1j): the circular state of S3 > 0): |conj(j).U|^2 / |j|^2 =
        (S0 + q1 S1 + q2 S2 + q3 S3) / 2 with (q1, q2, q3) the analyser's own normalised Stokes vector.  Linear in the
        Stokes images, computed on the host; (n_groups, nx, ny).  The axial component does not pass."""
        try:
            j = np.asarray(jones, dtype=complex).reshape(-1)
        except (TypeError, ValueError):
            j = np.zeros(0, dtype=complex)
        if j.shape != (2,) or not np.all(np.isfinite(j)) or not np.any(j != 0):
            raise ValueError(f"jones: two finite numbers (j1, j2), not both zero (got {jones!r})")
        norm = float(abs(j[0]) ** 2 + abs(j[1]) ** 2)
        cross = np.conj(j[0]) * j[1]
        q = ((abs(j[0]) ** 2 - abs(j[1]) ** 2) / norm, 2.0 * cross.real / norm, 2.0 * cross.imag / norm)
        s = self.stokes
        return 0.5 * (s[:, 0] + q[0] * s[:, 1] + q[1] * s[:, 2] + q[2] * s[:, 3])

    def to_pandas(self):
        """One row per group: what ``PSF.to_pandas`` gives, and strehl_apodized and throughput."""
        frame = super().to_pandas()
        frame["strehl_apodized"], frame["throughput"] = self.strehl_apodized, self.throughput
        return frame


class MTF:
    """What ``DeviceFrame.mtf`` returns (numpy arrays).  ``otf`` (n_groups, n_focus, n_azimuths, n_frequencies),
    complex; ``mtf`` = |otf| and ``ptf`` = arg otf (radians, about the group's centre); ``frequencies`` (cycles per world
    unit), ``azimuths`` (degrees) and ``focus`` (shifts along the axis); per group ``centre`` (n_groups, 3), ``n_rays``
    (rays summed), ``n_missed`` (rays left out) and ``sum_weights``.  A group without rays is NaN throughout."""

    def __init__(self, otf, record, frequencies, azimuths, focus):
        self.otf = np.asarray(otf)
        self.mtf, self.ptf = np.abs(self.otf), np.angle(self.otf)
        self.frequencies = np.asarray(frequencies, dtype=float)
        self.azimuths = np.asarray(azimuths, dtype=float)
        self.focus = np.asarray(focus, dtype=float)
        self.record = np.asarray(record, dtype=float)
        self.centre, self.sum_weights = self.record[:, :3], self.record[:, 3]
        self.n_rays = np.nan_to_num(self.record[:, 4]).astype(np.int64)
        self.n_missed = np.nan_to_num(self.record[:, 5]).astype(np.int64)

    def to_pandas(self):
        """Long form: one row per (source_id, focus, azimuth, frequency) with its mtf and ptf."""
        g, f, a, n = self.otf.shape
        index = np.indices((g, f, a, n)).reshape(4, -1)
        return pd.DataFrame({"source_id": index[0], "focus": self.focus[index[1]], "azimuth": self.azimuths[index[2]],
                             "frequency": self.frequencies[index[3]], "mtf": self.mtf.reshape(-1),
                             "ptf": self.ptf.reshape(-1)})

    def best_focus(self, frequency=None, azimuths=None):
        """Per group, the focus shift that maximises the MTF averaged over ``azimuths`` (None: all; else values of
        ``self.azimuths``) at ``frequency`` (a value of ``self.frequencies``; None: averaged over all of them).  The
        best sampled plane, refined by the vertex of the parabola through it and its two neighbours when it is not at
        an end of the scan.  NaN for a group without rays."""
        a_index = slice(None) if azimuths is None else _positions(self.azimuths, azimuths, "azimuths")
        f_index = slice(None) if frequency is None else _positions(self.frequencies, [frequency], "frequency")
        merit = self.mtf[:, :, a_index][:, :, :, f_index].mean(axis=(2, 3))  # (groups, planes)
        return _best_plane(self.focus, merit)


class MTFGradient:
    """What ``Sensitivity.mtf_gradient`` returns (numpy arrays), G groups, K parameters, F focus shifts, A azimuths, N
    frequencies.  ``otf`` (G, F, A, N) complex and ``mtf`` = |otf|, over the rays summed; ``dotf`` (G, K, F, A, N) complex,
    d(otf)/d(parameter k), and ``dotf_dfocus`` (G, F, A, N), d(otf)/d(focus shift); ``dmtf`` = Re(conj(otf) dotf) / |otf|
    (G, K, F, A, N), ``dmtf_dfocus``, and ``dptf`` = Im(conj(otf) dotf) / |otf|^2, the derivative of the phase in radians;
    all three NaN where |otf| = 0.  ``reference``: "fixed" (the centre held fixed) or "centroid" (it follows the group's
    centroid: ``dotf`` and ``dptf`` differ, ``dmtf`` does not but for rounding).  Per group ``centre`` (G, 3),
    ``centroid_gradient`` (G, K, 3) (d(centroid of the rays summed)/d(parameter)), ``sum_weights``, ``n_rays`` (rays
    summed), ``n_missed`` (left out by the MTF's rule), ``n_unfollowed`` (a Jacobian or slope that is not finite);
    ``record`` is the device's (G, 7 + 3 K) block.  ``frequencies``, ``azimuths``, ``focus``, ``parameters``.  A group
    without rays is NaN throughout."""

    def __init__(self, otf, dotf, record, frequencies, azimuths, focus, axes, parameters, reference="fixed"):
        self.otf = np.asarray(otf)
        self.frequencies = np.asarray(frequencies, dtype=float)
        self.azimuths = np.asarray(azimuths, dtype=float)
        self.focus = np.asarray(focus, dtype=float)
        self.parameters = tuple(parameters)
        self.reference = reference
        K = self.n_parameters = len(self.parameters)
        self.record = np.asarray(record, dtype=float)
        self.centre, self.sum_weights = self.record[:, :3], self.record[:, 3]
        self.n_rays, self.n_missed, self.n_unfollowed = (np.nan_to_num(self.record[:, k]).astype(np.int64) for k in (4, 5, 6))
        self.centroid_gradient = self.record[:, 7:].reshape(-1, K, 3)
        dotf = np.asarray(dotf)
        self.dotf, self.dotf_dfocus = dotf[:, :K], dotf[:, K]
        if reference == "centroid":  # (the centre follows the centroid: the phase of the shift, and the plane's own motion)
            a, e1, e2 = (np.asarray(axes, dtype=float)[k:k + 3] for k in (0, 3, 6))
            angle = np.radians(self.azimuths)
            kc, ks = np.cos(angle)[:, None] * self.frequencies, np.sin(angle)[:, None] * self.frequencies  # (A, N)
            dc = self.centroid_gradient
            shift = (dc @ e1)[:, :, None, None] * kc + (dc @ e2)[:, :, None, None] * ks  # (G, K, A, N)
            self.dotf = (self.dotf + 2j * np.pi * shift[:, :, None] * self.otf[:, None]
                         + (dc @ a)[:, :, None, None, None] * self.dotf_dfocus[:, None])
        self.mtf = np.abs(self.otf)
        with np.errstate(invalid="ignore", divide="ignore"):
            size = np.where(self.mtf > 0, self.mtf, np.nan)
            turned = np.conj(self.otf)[:, None] * self.dotf
            self.dmtf = turned.real / size[:, None]
            self.dptf = turned.imag / (size * size)[:, None]
            self.dmtf_dfocus = (np.conj(self.otf) * self.dotf_dfocus).real / size

    def to_pandas(self):
        """Long form: one row per (source_id, focus, azimuth, frequency) with its mtf, ``dmtf_dfocus`` and, per
        parameter k, ``dmtf_k`` and ``dptf_k``."""
        g, f, a, n = self.otf.shape
        index = np.indices((g, f, a, n)).reshape(4, -1)
        data = {"source_id": index[0], "focus": self.focus[index[1]], "azimuth": self.azimuths[index[2]],
                "frequency": self.frequencies[index[3]], "mtf": self.mtf.reshape(-1),
                "dmtf_dfocus": self.dmtf_dfocus.reshape(-1)}
        for k in range(self.n_parameters):
            data[f"dmtf_{k}"] = self.dmtf[:, k].reshape(-1)
            data[f"dptf_{k}"] = self.dptf[:, k].reshape(-1)
        return pd.DataFrame(data)

    def step(self, damping=0.0, target=1.0, focus=0.0):
        """Per group the change of the parameters that brings the MTF of the plane ``focus`` (a value of ``self.focus``)
        closest to ``target`` to first order: Gauss-Newton on the residuals ``target - mtf`` over that plane's azimuths
        and frequencies with ``dmtf`` as the Jacobian, the solution of (N + damping diag(N)) dp = rhs through
        ``solve_normal_equations`` (the minimum-norm one where the outputs cannot tell the parameters apart).
        (groups, K); NaN for a group without rays or with an output whose |otf| is 0."""
        if not (np.isfinite(damping) and damping >= 0):
            raise ValueError("damping: a number >= 0")
        if not np.isfinite(target):
            raise ValueError("target: a finite number")
        plane = _positions(self.focus, [focus], "focus")[0]
        K = self.n_parameters
        upper = np.triu_indices(K)
        packed = np.zeros((len(self.otf), len(upper[0]) + K + 3))
        for g in range(len(packed)):
            jac = self.dmtf[g, :, plane].reshape(K, -1).T  # (outputs, K)
            residual = (target - self.mtf[g, plane]).reshape(-1)
            if not np.all(np.isfinite(jac)) or not np.all(np.isfinite(residual)):
                continue
            normal = jac.T @ jac / len(residual)
            a = normal + damping * np.diag(np.diag(normal))
            packed[g, :len(upper[0])] = a[upper]
            packed[g, len(upper[0]):len(upper[0]) + K] = jac.T @ residual / len(residual)
            packed[g, -3] = len(residual)
        return solve_normal_equations(packed, K)[0]


class PSFGradient:
    """What ``Sensitivity.psf_gradient`` returns (numpy arrays), G groups, K parameters, L wavelengths.  ``image``
    (G, nx, ny) and ``image_by_wavelength`` (G, L, nx, ny): the normalised Huygens image over the rays kept, indexed as
    ``PSF.image`` is; ``dimage`` (G, K, nx, ny) and ``dimage_by_wavelength`` (G, K, L, nx, ny): its derivative per unit
    of parameter k; ``amplitude`` (G, L, nx, ny) and ``damplitude`` (G, K, L, nx, ny), complex: U_l and dU_l,k of
    include/prt.h (not normalised); ``strehl`` (G) and ``dstrehl`` (G, K): the image and its derivative at P; ``u`` (nx)
    and ``v`` (ny): the pixel centres; per group and wavelength ``n_rays`` (rays kept), ``n_missed`` (left out by the
    PSF's rule) and ``n_unfollowed`` (a derivative that is not finite); ``record`` is the device's (G, L, 5) block;
    ``follow``: "ray" or "pupil"; ``wavelengths`` (micrometres), ``parameters``, ``wavefront``.  A group without kept
    rays is NaN throughout."""

    def __init__(self, amplitude, damplitude, image_by_wavelength, dimage_by_wavelength, strehl, record, wavelengths,
                 world_unit_um, pixels, pixel_size, centre, f_number, wavefront, parameters, follow):
        self.amplitude, self.damplitude = np.asarray(amplitude), np.asarray(damplitude)
        self.image_by_wavelength, self.dimage_by_wavelength = image_by_wavelength, dimage_by_wavelength
        self.image, self.dimage = image_by_wavelength.sum(axis=1), dimage_by_wavelength.sum(axis=2)
        strehl = np.asarray(strehl, dtype=float)
        self.strehl, self.dstrehl = strehl[:, 0], strehl[:, 1:]
        self.record, self.wavelengths = np.asarray(record, dtype=float), np.asarray(wavelengths, dtype=float)
        self.world_unit_um, self.pixel_size, self.centre = world_unit_um, pixel_size, centre
        self.f_number, self.wavefront, self.follow = f_number, wavefront, follow
        self.parameters = tuple(parameters)
        self.n_parameters = len(self.parameters)
        nx, ny = pixels
        self.u = centre[0] + (np.arange(nx) - 0.5 * (nx - 1)) * pixel_size[0]
        self.v = centre[1] + (np.arange(ny) - 0.5 * (ny - 1)) * pixel_size[1]
        self.n_rays, self.n_missed, self.n_unfollowed = (self.record[:, :, k].astype(np.int64) for k in (0, 1, 2))

    def to_pandas(self):
        """One row per group: strehl, ``dstrehl_k`` per parameter k, f_number, n_rays, n_missed, n_unfollowed."""
        data = {"strehl": self.strehl}
        for k in range(self.n_parameters):
            data[f"dstrehl_{k}"] = self.dstrehl[:, k]
        data.update(f_number=self.f_number, n_rays=self.n_rays.sum(axis=1), n_missed=self.n_missed.sum(axis=1),
                    n_unfollowed=self.n_unfollowed.sum(axis=1))
        frame = pd.DataFrame(data)
        frame.index.name = "source_id"
        return frame

    def step(self, damping=0.0, target=None):
        """Per group the change of the parameters that brings the image closest to ``target`` to first order:
        Gauss-Newton on the residuals ``target - image`` over the pixels with ``dimage`` as the Jacobian, the solution of
        (N + damping diag(N)) dp = rhs through ``solve_normal_equations`` (the minimum-norm one where the pixels cannot
        tell the parameters apart).  ``target``: a (groups, nx, ny) array, or a ``PSF`` on the same grid -- a measured
        star image, say.  (groups, K); NaN for a group without rays."""
        if not (np.isfinite(damping) and damping >= 0):
            raise ValueError("damping: a number >= 0")
        if isinstance(target, PSF):
            if target.image.shape != self.image.shape or not (np.array_equal(target.u, self.u) and np.array_equal(target.v, self.v)):
                raise ValueError("target: a PSF on the same groups and pixel grid (pixels, pixel_size, centre)")
            target = target.image
        if target is None:
            raise ValueError("target: a (groups, nx, ny) array or a PSF on the same grid")
        wanted = np.asarray(target, dtype=float)
        if wanted.shape != self.image.shape:
            raise ValueError(f"target: shape {self.image.shape} (got {wanted.shape})")
        K = self.n_parameters
        upper = np.triu_indices(K)
        packed = np.zeros((len(self.image), len(upper[0]) + K + 3))
        for g in range(len(packed)):
            jac = self.dimage[g].reshape(K, -1).T  # (pixels, K)
            residual = (wanted[g] - self.image[g]).reshape(-1)
            if not np.all(np.isfinite(jac)) or not np.all(np.isfinite(residual)):
                continue
            normal = jac.T @ jac / len(residual)
            a = normal + damping * np.diag(np.diag(normal))
            packed[g, :len(upper[0])] = a[upper]
            packed[g, len(upper[0]):len(upper[0]) + K] = jac.T @ residual / len(residual)
            packed[g, -3] = len(residual)
        return solve_normal_equations(packed, K)[0]


class EnclosedEnergy:
    """What ``DeviceFrame.enclosed_energy`` returns (numpy arrays).  ``energy`` (n_groups, n_focus, n_radii): the
    fraction of the energy within each of ``radii``; ``radius`` (n_groups, n_focus, n_fractions): the radius (half-width
    for a square or a slit) that holds each of ``fractions``, a ray's own distance; ``focus`` (shifts along the axis)
    and ``shape``; per group ``centre`` (n_groups, 3), ``centroid_shift`` (n_groups, 2, 2): pbar and sbar, the weighted
    means of p and of the slope s about the centre (the centroid of the plane at shift delta is pbar + delta sbar);
    ``n_rays`` (rays used), ``n_missed`` (rays left out) and ``sum_weights``.  A group without rays, or whose weights
    are all zero, is NaN throughout."""

    def __init__(self, energy, radius, record, radii, fractions, focus, shape="circle"):
        self.energy, self.radius = np.asarray(energy, dtype=float), np.asarray(radius, dtype=float)
        self.radii = np.asarray(radii, dtype=float)
        self.fractions = np.asarray(fractions, dtype=float)
        self.focus = np.asarray(focus, dtype=float)
        self.shape = shape
        self.record = np.asarray(record, dtype=float)
        self.centre, self.sum_weights = self.record[:, :3], self.record[:, 7]
        self.centroid_shift = self.record[:, 3:7].reshape(-1, 2, 2)
        self.n_rays = np.nan_to_num(self.record[:, 8]).astype(np.int64)
        self.n_missed = np.nan_to_num(self.record[:, 9]).astype(np.int64)

    def to_pandas(self):
        """Long form: one row per (source_id, focus, quantity, value) -- quantity "energy" with its radius in
        ``radius`` and the enclosed fraction in ``energy``, then quantity "radius" likewise for each of ``fractions``."""
        parts = []
        for name, block, radius_of, energy_of in (
                ("energy", self.energy, lambda j, v: self.radii[j], lambda j, v: v),
                ("radius", self.radius, lambda j, v: v, lambda j, v: self.fractions[j])):
            index = np.indices(block.shape).reshape(3, -1)
            values = block.reshape(-1)
            parts.append(pd.DataFrame({"source_id": index[0], "focus": self.focus[index[1]], "quantity": name,
                                       "radius": radius_of(index[2], values), "energy": energy_of(index[2], values)}))
        return pd.concat(parts, ignore_index=True)

    def best_focus(self, fraction=None):
        """Per group, the focus shift of the smallest enclosed radius at ``fraction`` (a value of ``self.fractions``;
        None: the mean over all of them).  The best sampled plane, refined by the vertex of the parabola through it
        and its two neighbours when it is not at an end of the scan (``MTF.best_focus``'s rule).  NaN for a group
        without rays."""
        if not len(self.fractions):
            raise ValueError("fraction: this result holds no enclosed radius (it was made without fractions)")
        index = slice(None) if fraction is None else _positions(self.fractions, [fraction], "fraction")
        return _best_plane(self.focus, -self.radius[:, :, index].mean(axis=2))


def _best_plane(focus, merit):
    """Per group the focus shift of the largest merit (groups, planes): the best sampled plane, refined by the vertex
    of the parabola through it and its two neighbours when it is interior.  NaN where no plane is finite."""
    order = np.argsort(focus, kind="stable")
    x, merit = focus[order], merit[:, order]
    best = np.full(len(merit), np.nan)
    for g, y in enumerate(merit):
        if not np.any(np.isfinite(y)):
            continue
        k = int(np.nanargmax(y))
        best[g] = x[k]
        if 0 < k < len(x) - 1 and np.all(np.isfinite(y[k - 1:k + 2])):
            (x0, x1, x2), (y0, y1, y2) = x[k - 1:k + 2], y[k - 1:k + 2]
            a = ((y2 - y1) / (x2 - x1) - (y1 - y0) / (x1 - x0)) / (x2 - x0)
            if a < 0:
                slope = (y1 - y0) / (x1 - x0) - a * (x0 + x1)  # (y = a x^2 + slope x + c)
                best[g] = float(np.clip(-slope / (2 * a), x0, x2))
    return best


class RayAberrations:
    """What ``DeviceFrame.ray_aberrations`` returns.  Per ray used, in row order (device tensors): ``pupil`` (n, 2), the
    normalised launch coordinate p; ``transverse`` (n, 2), eps about the group's reference point; ``slope`` (n, 2), s;
    ``longitudinal`` (n), la (NaN for a ray parallel to the axis); ``rows`` (n), the ray's row number in the frame;
    ``launch`` (n, 2), the launch coordinate h itself, and ``group`` (n).  Per group (numpy arrays): ``centre``
    (n_groups, 3), ``pupil_radius`` (rho), ``n_rays``, ``n_missed``, ``n_longitudinal`` (rays with a finite la),
    ``chief_row`` (-1: none), ``sum_weights``, ``coefficients`` (n_groups, 4, J) -- Noll's Z1..ZJ fitted to eps1, eps2,
    s1, s2 over p --, ``rank`` of the fit's normal equations and ``residual`` (n_groups, 4), the weighted RMS of what the
    fit leaves of each target; ``record`` (n_groups, 16), ``normal`` and ``zones`` (n_groups, n_zones, 6): the device's
    sums (include/prt.h)."""

    def __init__(self, rays, rows, record, normal, zones, terms, h=None, group=None):
        self.rays, self.rows, self.terms = rays, rows, int(terms)
        self.pupil, self.transverse, self.slope, self.longitudinal = rays[:, 0:2], rays[:, 2:4], rays[:, 4:6], rays[:, 6]
        self.record = np.atleast_2d(np.asarray(record, dtype=float))
        self.normal = np.atleast_2d(np.asarray(normal, dtype=float))
        self.zones = np.asarray(zones, dtype=float).reshape(len(self.record), -1, 6)
        self.launch, self.group = h, group
        r = self.record
        self.centre, self.pupil_radius = r[:, 0:3], r[:, 3]
        self.n_rays, self.n_missed = r[:, 4].astype(np.int64), r[:, 5].astype(np.int64)
        self.n_longitudinal, self.chief_row = r[:, 6].astype(np.int64), r[:, 7].astype(np.int64)
        self.sum_weights = r[:, 8]
        tri = self.terms * (self.terms + 1) // 2
        n = len(r)
        self.coefficients = np.full((n, 4, self.terms), np.nan)
        self.rank = np.zeros(n, dtype=np.int64)
        for k in range(4):  # (one right-hand side at a time through the wavefront's solver)
            system = np.concatenate([self.normal[:, :tri], self.normal[:, tri + k * self.terms:tri + (k + 1) * self.terms],
                                     self.normal[:, -1:], np.zeros((n, 2))], axis=1)
            self.coefficients[:, k], self.rank = solve_normal_equations(system, self.terms)
        # what the fit leaves: sum w t^2 - c.(Z^T W t), for eps (both components, about C) and s (raw)
        rhs = self.normal[:, tri:tri + 4 * self.terms].reshape(n, 4, self.terms)
        explained = (self.coefficients * rhs).sum(axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            left_eps = np.maximum(r[:, 13] - explained[:, 0] - explained[:, 1], 0.0) / r[:, 8]
            left_s = np.maximum(r[:, 15] - explained[:, 2] - explained[:, 3], 0.0) / r[:, 8]
        self.residual = np.stack([np.sqrt(left_eps), np.sqrt(left_s)], axis=1)

    def _moments(self):
        r = self.record
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(r[:, 8] > 0, r[:, 8], np.nan)
            m_eps, m_s = r[:, 9:11] / w[:, None], r[:, 11:13] / w[:, None]
            ee = r[:, 13] / w - (m_eps ** 2).sum(axis=1)
            es = r[:, 14] / w - (m_eps * m_s).sum(axis=1)
            ss = r[:, 15] / w - (m_s ** 2).sum(axis=1)
        return ee, es, ss

    def rms_radius(self, focus=0.0):
        """Per group, the RMS spot radius about the spot's own centroid at the plane shifted by ``focus`` along the
        axis: sqrt(var eps + 2 focus cov(eps, s) + focus^2 var s), from the group sums."""
        ee, es, ss = self._moments()
        return np.sqrt(np.maximum(ee + 2.0 * focus * es + focus * focus * ss, 0.0))

    def best_focus(self):
        """Per group, the shift along the axis that minimises the RMS spot radius, in closed form:
        -cov(eps, s) / var(s) (NaN when every ray has the same slope)."""
        _, es, ss = self._moments()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ss > 0, -es / ss, np.nan)

    def fan(self, azimuth_deg, samples=65, focus=0.0):
        """The fitted transverse aberration eps + focus * s along the pupil diameter at ``azimuth_deg`` (0: the
        tangential fan along e1; 90: the sagittal fan along e2): ``(t, along, across)`` with t the ``samples``
        positions from -1 to 1 on the diameter and, per group, the components of the aberration along the diameter
        and across it (arrays (n_groups, samples))."""
        t = np.linspace(-1.0, 1.0, int(samples))
        angle = np.radians(float(azimuth_deg))
        c, s = np.cos(angle), np.sin(angle)
        basis = zernike_basis(self.terms, np.abs(t), np.where(t >= 0, angle, angle + np.pi))  # (terms, samples)
        value = np.einsum("gkj,js->gks", self.coefficients, basis)
        e1 = value[:, 0] + focus * value[:, 2]
        e2 = value[:, 1] + focus * value[:, 3]
        return t, c * e1 + s * e2, -s * e1 + c * e2

    def longitudinal_curve(self):
        """The zonal curve of the longitudinal aberration (the notebook's cell 13 for any number of rays): a dict of
        arrays (n_groups, n_zones) -- ``radius`` (the zones' centres in world units, (zone + 1/2) / n_zones * rho),
        ``mean`` and ``std`` (weighted, over the zone's rays with a finite la; NaN for a zone without one), ``count``
        (those rays) and ``rays`` (all the zone's rays)."""
        z = self.zones
        n_zones = z.shape[1]
        centres = (np.arange(n_zones) + 0.5) / max(n_zones, 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(z[:, :, 1] > 0, z[:, :, 1], np.nan)
            mean = z[:, :, 2] / w
            std = np.sqrt(np.maximum(z[:, :, 3] / w - mean * mean, 0.0))
        return {"radius": centres[None, :] * self.pupil_radius[:, None], "mean": mean, "std": std,
                "count": z[:, :, 5].astype(np.int64), "rays": z[:, :, 0].astype(np.int64)}

    def to_pandas(self):
        """One row per ray used, in row order: row, source_id, radius (= h1) and h2, p1, p2, eps1, eps2, s1, s2 and
        focus (= la) -- ``table['radius'], table['focus']`` are the two columns the notebook's ``spherical_aberration()``
        returns."""
        from . import engine

        def host(x):
            return engine.to_host(x) if hasattr(x, "is_cuda") else np.asarray(x)

        rays = host(self.rays)
        rows = host(self.rows)
        group = np.zeros(len(rows), dtype=np.int64) if self.group is None else host(self.group)
        if self.launch is not None:
            h = host(self.launch)
        else:
            h = rays[:, 0:2] * self.pupil_radius[group][:, None]
        return pd.DataFrame({"row": rows, "source_id": group, "radius": h[:, 0], "h2": h[:, 1], "p1": rays[:, 0],
                             "p2": rays[:, 1], "eps1": rays[:, 2], "eps2": rays[:, 3], "s1": rays[:, 4], "s2": rays[:, 5],
                             "focus": rays[:, 6]})


class Paths:
    """The ray paths of a frame (``DeviceFrame.paths``): a tree of the prefixes of every ray's sequence of surfaces.

    ``sequences`` (a list of tuples in the canonical order: ascending as tuples), ``parent`` (-1 for a first surface),
    ``surface``, ``depth`` and ``subtree_size`` describe the ``n_nodes`` nodes; ``through``, ``ended``, ``dark``,
    ``energy_through`` and ``energy_ended`` are (n_groups, n_nodes) tables.  ``row_node`` (per row of the frame),
    ``ray_node`` and ``ray_last_row`` (per id, from ``id0``; -1 for an id without rows) are device tensors -- None on
    an object made by ``merge`` -- and ``rays`` / ``rows`` turn nodes into masks for ``frame.select``."""

    def __init__(self, parent, surface, depth, subtree_size, through, ended, dark, energy_through, energy_ended,
                 row_node=None, ray_node=None, ray_last_row=None, id0=0.0, n_bad_weight=0, n_rays=None, ids=None,
                 launched=None):
        self.parent = np.asarray(parent, dtype=np.int64)
        self.surface = np.asarray(surface)
        self.depth = np.asarray(depth, dtype=np.int64)
        self.subtree_size = np.asarray(subtree_size, dtype=np.int64)
        n = len(self.parent)
        self.through = np.asarray(through, dtype=np.int64).reshape(-1, n)
        self.ended = np.asarray(ended, dtype=np.int64).reshape(-1, n)
        self.dark = np.asarray(dark, dtype=np.int64).reshape(-1, n)
        self.energy_through = np.asarray(energy_through, dtype=np.float64).reshape(-1, n)
        self.energy_ended = np.asarray(energy_ended, dtype=np.float64).reshape(-1, n)
        self.row_node, self.ray_node, self.ray_last_row = row_node, ray_node, ray_last_row
        self.id0, self.n_bad_weight = id0, int(n_bad_weight)
        self.n_rays = int(self.ended.sum()) if n_rays is None else int(n_rays)
        self.launched = launched  # (rays per source, where the tracer knows it: trace_paths)
        self._ids = ids
        self.sequences = []
        for k in range(n):  # (a parent comes before its children)
            head = self.sequences[self.parent[k]] if self.parent[k] >= 0 else ()
            self.sequences.append(head + (self.surface[k].item() if hasattr(self.surface[k], "item") else self.surface[k],))
        self._number = {sequence: k for k, sequence in enumerate(self.sequences)}

    @property
    def n_nodes(self):
        return len(self.parent)

    @property
    def n_groups(self):
        return self.through.shape[0]

    def to_pandas(self):
        """One line per (source, node), with the node's sequence."""
        g, k = np.divmod(np.arange(self.n_groups * self.n_nodes), max(self.n_nodes, 1))
        return pd.DataFrame({"source_id": g, "node": k, "parent": self.parent[k], "depth": self.depth[k],
                             "surface": self.surface[k], "sequence": [self.sequences[n] for n in k],
                             "through": self.through.reshape(-1), "ended": self.ended.reshape(-1),
                             "dark": self.dark.reshape(-1), "energy_through": self.energy_through.reshape(-1),
                             "energy_ended": self.energy_ended.reshape(-1)})

    def complete(self):
        """The nodes where rays ended: the complete paths."""
        return np.flatnonzero(self.ended.sum(axis=0) > 0)

    def index(self, sequence):
        """The number of the node with this sequence of surfaces (ids or objects with ``get_id()``)."""
        key = tuple(_surface_id(item) for item in sequence)
        if key not in self._number:
            raise ValueError(f"no ray went through {key}")
        return self._number[key]

    def find(self, through=None, ends_at=None, avoids=None):
        """The numbers of the nodes whose sequence holds every surface of ``through``, ends at ``ends_at`` and holds
        none of ``avoids`` (each a surface id, an object with ``get_id()`` or several of them; None: no condition)."""
        need, stop, last = _surface_ids(through), _surface_ids(avoids), _surface_ids(ends_at)
        return np.array([k for k, sequence in enumerate(self.sequences)
                         if need <= set(sequence) and not (stop & set(sequence)) and (not last or sequence[-1] in last)],
                        dtype=np.int64)

    def _range(self, node, complete):
        node = int(node)
        if not 0 <= node < self.n_nodes:
            raise ValueError(f"node: 0 to {self.n_nodes - 1} (got {node})")
        return node, node + (1 if complete else int(self.subtree_size[node]))

    def rays(self, node, complete=True):
        """A device mask over the ids (from ``id0``): the rays whose complete path is ``node`` (a number or several),
        or, with complete=False, every ray whose path has the node as a prefix -- the range test
        ``node <= ray_node < node + subtree_size[node]``."""
        if self.ray_node is None:
            raise ValueError("this Paths holds no per-ray tensors (it was made by merge())")
        mask = None
        for k in np.atleast_1d(np.asarray(node)):
            lo, hi = self._range(k, complete)
            m = (self.ray_node >= lo) & (self.ray_node < hi)
            mask = m if mask is None else (mask | m)
        return mask if mask is not None else self.ray_node < -1

    def rows(self, node, complete=True):
        """The same as a mask over the frame's rows, for ``frame.select(...)``: every row of the rays ``rays`` picks."""
        picked = self.rays(node, complete)
        index = self._ids - self.id0
        return picked[index.long() if hasattr(index, "long") else np.asarray(index, dtype=np.int64)]

    def fates(self, launched=None):
        """Per source and final surface the rays that ended there, those of them that were absorbed (dark) and those
        that escaped or ran into the generation limit, with the energy of their last rows.  launched: the rays per
        source (a number or one per source; by default what ``trace_paths`` knows): the table then also gives, as
        surface -1, the rays that never met a surface -- launched minus the rays through the first surfaces."""
        launched = self.launched if launched is None else launched
        surfaces = sorted(set(self.surface[self.ended.sum(axis=0) > 0].tolist()))
        lines = []
        for g in range(self.n_groups):
            if launched is not None:
                missed = int(np.broadcast_to(np.asarray(launched), (self.n_groups,))[g]) - int(
                    self.through[g, self.depth == 0].sum())
                lines.append((g, -1, missed, 0, missed, 0.0))
            for surface in surfaces:
                at = self.surface == surface
                ended, dark = int(self.ended[g, at].sum()), int(self.dark[g, at].sum())
                if ended:
                    lines.append((g, surface, ended, dark, ended - dark, float(self.energy_ended[g, at].sum())))
        return pd.DataFrame(lines, columns=["source_id", "surface", "ended", "dark", "escaped", "energy_ended"])

    def merge(self, labels, collapse_repeats=False):
        """A coarser tree, on the host: every surface relabelled through the dict ``labels`` (surface id -> a
        component's label, say; a surface that is not in it keeps its id), consecutive repeats of a label dropped when
        ``collapse_repeats``, and the tables of the nodes that fall together added (a ray counts once in a merged
        node: where it entered it).  Returns a ``Paths`` without device tensors; its ``node_map`` gives each old
        node's new number."""
        relabelled = []
        for sequence in self.sequences:
            out = []
            for surface in sequence:
                label = labels.get(surface, surface)
                if not (collapse_repeats and out and out[-1] == label):
                    out.append(label)
            relabelled.append(tuple(out))
        merged = sorted(set(relabelled))
        number = {sequence: k for k, sequence in enumerate(merged)}
        node_map = np.array([number[sequence] for sequence in relabelled], dtype=np.int64)
        n = len(merged)
        tables = [np.zeros((self.n_groups, n), dtype=t.dtype)
                  for t in (self.through, self.ended, self.dark, self.energy_through, self.energy_ended)]
        for k, m in enumerate(node_map):
            entered = self.parent[k] < 0 or node_map[self.parent[k]] != m
            for table, old in zip(tables, (self.through, self.ended, self.dark, self.energy_through, self.energy_ended)):
                if entered or old is self.ended or old is self.dark or old is self.energy_ended:
                    table[:, m] += old[:, k]
        parent = np.array([number[sequence[:-1]] if len(sequence) > 1 else -1 for sequence in merged], dtype=np.int64)
        size = np.ones(n, dtype=np.int64)
        for k in range(n - 1, -1, -1):
            if parent[k] >= 0:
                size[parent[k]] += size[k]
        surface = np.empty(n, dtype=object)
        surface[:] = [sequence[-1] for sequence in merged]
        if n and all(isinstance(v, (int, np.integer)) for v in surface):
            surface = surface.astype(np.int64)
        out = Paths(parent, surface, [len(sequence) - 1 for sequence in merged], size, *tables, id0=self.id0,
                    n_bad_weight=self.n_bad_weight, n_rays=self.n_rays, launched=self.launched)
        out.node_map = node_map
        return out


class Fresnel:
    """What ``DeviceFrame.fresnel`` returns.  ``transmittance``: a device tensor, per row of the frame the share of the
    ray's launch energy left on that row's segment (1 at generation 0; NaN for a ray past an invalid interface);
    ``field``: None, or a device (6, n_rows) tensor, Ea then Eb by component; the counters ``n_reflections`` (interfaces
    with equal indices and a deviated ray: their retardance is not modelled), ``n_lossless`` (interfaces at a surface of
    the ``lossless`` list), ``n_undeviated`` and ``n_invalid`` (rays); ``polarization`` and ``lossless`` as given.
    From ``fresnel(coatings=...)`` or a complex ``polarization``: ``field`` is complex128, and ``n_coated`` (interfaces
    at a coated surface) and ``n_tir`` (of them, total internal reflections: a real far index below the Snell invariant)
    are counted as well; both are 0 otherwise."""

    def __init__(self, frame, transmittance, field, record, polarization=None, lossless=(), coatings=None):
        self.frame, self.transmittance, self.field = frame, transmittance, field
        self.n_reflections, self.n_lossless, self.n_undeviated, self.n_invalid = (int(v) for v in record[:4])
        self.n_coated, self.n_tir = (int(v) for v in record[4:6]) if len(record) >= 6 else (0, 0)
        self.polarization, self.lossless, self.coatings = polarization, tuple(lossless), coatings
        self.launch_states = None  # ("per_ray": the two states of fresnel(polarization=None); see uniform_states)
        self._paths = {}

    def uniform_states(self, polarization=None):
        """A ``Fresnel`` with the same transmittance whose two states are uniform across the beam, for sums that are
        coherent over the rays (``DeviceFrame.psf(fresnel=)``).  ``fresnel(polarization=None)`` launches every ray with
        two orthogonal fields in a transverse basis made from the ray's own direction (the world axis of its smallest
        component), which is all the per-ray transmittance needs; across a cone that basis jumps from ray to ray, so
        ``Ea`` alone is not one polarisation state of the beam.  The pass is linear in the launch field, so the fields
        of any other launch state are combinations of ``Ea`` and ``Eb``: the new ``Ea`` belongs to the launch field of
        ``polarization`` (a real world vector; None: the world axis most nearly perpendicular to the mean launch
        direction) taken perpendicular to each ray's launch direction u0 and normalised, as ``fresnel(polarization=)``
        launches it, and the new ``Eb`` to u0 x that.  A rotation per ray: ``|Ea|^2 + |Eb|^2`` is unchanged.  Rows of a
        ray without a generation-0 row are NaN."""
        import torch

        if self.field is None:
            raise ValueError("uniform_states: the fields were not kept (fresnel(fields=True))")
        if self.polarization is not None:
            raise ValueError("uniform_states: this Fresnel has one state (polarised input)")
        rows, counts = self.frame.rows, self.frame.rows_per_generation
        if not counts or sum(counts) != rows.shape[1]:
            raise ValueError("uniform_states needs the whole frame of a trace")
        n0 = int(counts[0])
        ids = rows[_INDEX["id"]]
        slot = (ids - ids.min()).long() if rows.shape[1] else ids.long()
        table = torch.full((int(slot.max()) + 1 if rows.shape[1] else 1,), -1, dtype=torch.long, device=rows.device)
        table[slot[:n0]] = torch.arange(n0, device=rows.device)
        launch = table[slot]  # (per row: the generation-0 row of its ray)
        known = launch >= 0
        launch = launch.clamp(min=0)
        u0 = torch.stack([rows[_INDEX[name]][launch] for name in ("x_tilt", "y_tilt", "z_tilt")])
        u0 = u0 / torch.sqrt((u0 * u0).sum(dim=0))
        if polarization is None:
            mean = u0[:, known].mean(dim=1).abs()
            g = torch.nn.functional.one_hot(torch.argmin(mean), 3).to(u0.dtype)
        else:
            g = torch.as_tensor(np.asarray(polarization, dtype=np.float64).reshape(-1), device=rows.device)
            if g.shape != (3,) or not bool(torch.isfinite(g).all()) or not bool((g != 0).any()):
                raise ValueError("uniform_states: polarization is a real world vector of three finite numbers, not all zero")
        g1 = g[:, None] - (g[:, None] * u0).sum(dim=0) * u0
        g1 = g1 / torch.sqrt((g1 * g1).sum(dim=0))
        g2 = torch.linalg.cross(u0, g1, dim=0)
        ea, eb = self.field[:3], self.field[3:6]
        base_a, base_b = (x[:, launch].real if x.is_complex() else x[:, launch] for x in (ea, eb))
        nan = torch.full_like(self.transmittance, float("nan"))
        weights = [torch.where(known, (base * axis).sum(dim=0), nan) for axis in (g1, g2) for base in (base_a, base_b)]
        field = torch.cat([weights[0] * ea + weights[1] * eb, weights[2] * ea + weights[3] * eb])
        out = Fresnel(self.frame, self.transmittance, field, np.array([self.n_reflections, self.n_lossless,
                      self.n_undeviated, self.n_invalid, self.n_coated, self.n_tir]), polarization=None,
                      lossless=self.lossless, coatings=self.coatings)
        out.launch_states = "uniform"
        return out

    def stokes(self, rows=None):
        """Per row (``rows``: an index tensor or slice; None: all) the Stokes parameters S0..S3 of ``Ea`` -- the field of
        polarised input -- as a (4, n) device tensor.  The transverse basis is the one launch fields use: for the row's
        direction u, e1 = u x e normalised with e the world axis of the smallest |u| component (ties to the first),
        e2 = u x e1; with E1 = Ea.e1, E2 = Ea.e2: S0 = |E1|^2 + |E2|^2, S1 = |E1|^2 - |E2|^2, S2 = 2 Re(conj(E1) E2),
        S3 = 2 Im(conj(E1) E2).  Needs ``fields=True``."""
        import torch

        if self.field is None:
            raise ValueError("stokes: the fields were not kept (fresnel(fields=True))")
        pick = slice(None) if rows is None else rows
        u = torch.stack([self.frame[name] for name in ("x_tilt", "y_tilt", "z_tilt")])[:, pick]
        u = u / torch.sqrt((u * u).sum(dim=0))
        magnitude = u.abs()
        axis = torch.zeros(u.shape[1], dtype=torch.long, device=u.device)
        least = magnitude[0].clone()
        second = magnitude[1] < least
        axis[second] = 1
        least = torch.where(second, magnitude[1], least)
        axis[magnitude[2] < least] = 2
        e = torch.nn.functional.one_hot(axis, 3).T.to(u.dtype)
        e1 = torch.linalg.cross(u, e, dim=0)
        e1 = e1 / torch.sqrt((e1 * e1).sum(dim=0))
        e2 = torch.linalg.cross(u, e1, dim=0)
        ea = self.field[:3][:, pick].to(torch.complex128)
        c1, c2 = (ea * e1).sum(dim=0), (ea * e2).sum(dim=0)
        cross = torch.conj(c1) * c2
        p1, p2 = c1.real ** 2 + c1.imag ** 2, c2.real ** 2 + c2.imag ** 2
        return torch.stack([p1 + p2, p1 - p2, 2.0 * cross.real, 2.0 * cross.imag])

    def to_pandas(self):
        """One line per row of the frame: generation, id, surface, intensity, transmittance (and the fields)."""
        from . import engine

        table = pd.DataFrame({name: engine.to_host(self.frame[name]) for name in ("generation", "id", "surface", "intensity")})
        table["transmittance"] = engine.to_host(self.transmittance)
        if self.field is not None:
            for k, name in enumerate(("ea_x", "ea_y", "ea_z", "eb_x", "eb_y", "eb_z")):
                table[name] = engine.to_host(self.field[k].contiguous())
        return table

    def apply(self):
        """A new whole frame, a copy of the rows with ``intensity`` replaced by ``intensity * transmittance`` (one
        multiply per row), with the same ``rows_per_generation``: every pass that weighs by intensity then sees the
        losses.  The frame the transmittance was computed on is left as it is."""
        rows = self.frame.rows.clone()
        rows[_INDEX["intensity"]] = self.frame.rows[_INDEX["intensity"]] * self.transmittance
        return DeviceFrame(rows, self.frame.rows_per_generation, self.frame.written)

    def transmission(self, surface, rays_per_source=None):
        """Per source (``id // rays_per_source``; None: one), the energy that arrives at ``surface`` (an id or an object
        with ``get_id()``) in the applied frame over the energy launched -- the intensity of the generation-0 rows of
        the original frame.  Both are ``paths()``' exact integer sums, so the ratio is the same bits on every run."""
        wanted = _surface_id(surface)
        if rays_per_source not in self._paths:
            options = dict(weights="intensity", rays_per_source=rays_per_source)
            self._paths[rays_per_source] = (self.apply().paths(**options), self.frame.paths(**options))
        applied, original = self._paths[rays_per_source]
        arrived = applied.energy_through[:, applied.surface == wanted].sum(axis=1)
        launched = original.energy_through[:, original.depth == 0].sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return arrived / launched


class Motion:
    """One parameter of ``DeviceFrame.sensitivity``: a rigid motion of a part, per unit of the parameter.  ``part``: a
    surface id, an object with ``get_id()`` or a component (every leaf surface of it moves: ``surface_ids``).
    ``translate``: the velocity, in world length per unit parameter; ``rotate``: an axis scaled to radians per unit
    parameter (right-handed), about ``pivot`` (default: the part's position; a bare id has none, (0, 0, 0) then).  A point
    x of the part moves with u = translate + rotate x (x - pivot).  At most 64 surface ids."""

    def __init__(self, part, translate=(0.0, 0.0, 0.0), rotate=(0.0, 0.0, 0.0), pivot=None):
        if hasattr(part, "surface_ids"):
            ids = [int(sid) for sid, _ in part.surface_ids]
        elif hasattr(part, "get_id"):
            ids = [int(part.get_id())]
        else:
            try:
                ids = [int(part)]
                if ids[0] != part:
                    raise TypeError
            except (TypeError, ValueError):
                raise ValueError(f"Motion: part is an id, an object with get_id() or a component (got {part!r})") from None
        if len(set(ids)) > 64:
            raise ValueError(f"Motion: at most 64 surface ids a parameter (got {len(set(ids))})")
        if pivot is None:
            pivot = (0.0, 0.0, 0.0)
            if hasattr(part, "get_position"):
                pivot = np.asarray(part.get_position(), dtype=float).reshape(-1)[:3]
        vectors = []
        for name, value in (("translate", translate), ("rotate", rotate), ("pivot", pivot)):
            try:
                vector = np.asarray(value, dtype=float).reshape(-1)
            except (TypeError, ValueError):
                vector = np.zeros(0)
            if vector.shape != (3,) or not np.all(np.isfinite(vector)):
                raise ValueError(f"Motion: {name} is three finite numbers (got {value!r})")
            vectors.append(vector)
        self.surface_ids = tuple(sorted(set(ids)))
        self.translate, self.rotate, self.pivot = vectors
        self.twist = np.concatenate(vectors)

    def __repr__(self):
        return (f"Motion(surfaces={self.surface_ids}, translate={tuple(self.translate)}, rotate={tuple(self.rotate)}, "
                f"pivot={tuple(self.pivot)})")


def _expm(generator):
    """exp of a small square matrix: scaling and squaring around a Taylor series (the 4x4 generators of ``Deformation``)."""
    g = np.asarray(generator, dtype=float)
    squarings = max(0, int(np.ceil(np.log2(max(np.linalg.norm(g, 1), 1e-300)))) + 4)
    g = g / 2.0 ** squarings
    out, term = np.eye(len(g)), np.eye(len(g))
    for k in range(1, 20):
        term = term @ g / k
        out = out + term
    for _ in range(squarings):
        out = out @ out
    return out


class Deformation:
    """One parameter of ``DeviceFrame.sensitivity``, the general one: an affine deformation of a part, per unit of the
    parameter.  A point x of the part moves with u = translate + rotate x (x - pivot) + linear (x - pivot); ``linear`` is
    any 3x3 matrix in world coordinates (None: 0, a rigid motion, what a ``Motion`` is).  ``part`` and ``pivot`` are
    ``Motion``'s.  Every shape parameter of the five primitives is such a deformation, and the constructors say which:

    ``Deformation.radius(surface, keep=None)``     the radius of a sphere or cylinder leaf, in the primitive's own frame:
                                                   linear = A^-1 diag(1/R) A (A the 3x3 of the leaf's world-to-object
                                                   matrix, R its radius; a cylinder's axis is not scaled);
    ``Deformation.focus(paraboloid, keep=None)``   the focus f of a paraboloid leaf: x and y scaled at the rate 1/(2f);
    ``Deformation.stretch(part, axis, about=None)`` a scaling along a world axis (cylinder heights, cuboid sides, the
                                                   thickness of a slab): linear = e e^T, the parameter is the relative
                                                   elongation, so a slab of thickness t grows by t per unit.

    ``keep`` is a world point that stays where it is (the pivot): a lens vertex, so that the thickness does not change with
    the radius; by default the primitive's own origin (a sphere's centre, a paraboloid's vertex).  The leaves of a
    component are in ``component.surface_ids``, as (id, surface) pairs, left child first: a ``biconvex_lens`` gives the
    front sphere (the face towards -x, vertex at position - thickness / 2 along the axis), the back sphere and the
    aperture stock, in that order; the thickness of a lens is ``Deformation(back, translate=axis)``.

    ``matrix(amount)`` is the finite 4x4 world transform whose derivative at 0 is u: for a radius the exact scaling by
    (R + amount) / R about ``keep`` (for a focus by sqrt((f + amount) / f) in x and y), for a stretch the scaling by
    1 + amount along the axis, otherwise the matrix exponential of amount times the generator of u.  ``apply(amount)``
    transforms the part with it (the primitive keeps its own parameters: its transform carries the change, and a later
    ``radius`` is again measured in the primitive's own frame).  A Deformation describes the part as it stood when it was
    made: after a step, make the next iteration's anew."""

    def __init__(self, part, translate=(0.0, 0.0, 0.0), rotate=(0.0, 0.0, 0.0), linear=None, pivot=None):
        try:
            rigid = Motion(part, translate, rotate, pivot)
        except ValueError as error:
            raise ValueError(str(error).replace("Motion:", "Deformation:", 1)) from None
        if linear is None:
            linear = np.zeros((3, 3))
        try:
            linear = np.array(linear, dtype=float)
        except (TypeError, ValueError):
            linear = np.zeros(0)
        if linear.shape != (3, 3) or not np.all(np.isfinite(linear)):
            raise ValueError("Deformation: linear is a 3x3 matrix of finite numbers")
        self.part = part
        self.surface_ids = rigid.surface_ids
        self.translate, self.rotate, self.pivot, self.twist = rigid.translate, rigid.rotate, rigid.pivot, rigid.twist
        self.linear = linear
        self._finite = None

    @staticmethod
    def _leaf(surface, kinds, what):
        from .g3d import shapes

        kind = getattr(getattr(surface, "primitive", None), "kind", None)
        names = {shapes.SPHERE: "sphere", shapes.CYLINDER: "cylinder", shapes.PARABOLOID: "paraboloid"}
        if kind not in kinds:
            raise ValueError(f"Deformation.{what}: a leaf surface that is a {' or a '.join(names[k] for k in kinds)} "
                             f"(got {surface!r})")
        a = np.asarray(surface.get_object_transform(), dtype=float)[:3, :3]
        return kind, a, np.linalg.inv(a), float(surface.primitive.params[0])

    @classmethod
    def _scaling(cls, surface, keep, rate, factor):
        """The deformation whose own-frame scaling has the diagonal rate ``rate`` and the finite diagonal ``factor(amount)``."""
        a = np.asarray(surface.get_object_transform(), dtype=float)[:3, :3]
        back = np.linalg.inv(a)
        if keep is None:
            keep = np.asarray(surface.get_position(), dtype=float).reshape(-1)[:3]
        out = cls(surface, linear=back @ np.diag(rate) @ a, pivot=keep)

        def finite(amount):
            m = np.eye(4)
            m[:3, :3] = back @ np.diag(factor(amount)) @ a
            m[:3, 3] = out.pivot - m[:3, :3] @ out.pivot
            return m

        out._finite = finite
        return out

    @classmethod
    def radius(cls, surface, keep=None):
        from .g3d import shapes

        kind, _, _, r = cls._leaf(surface, (shapes.SPHERE, shapes.CYLINDER), "radius")
        z = 1.0 if kind == shapes.SPHERE else 0.0

        def factor(amount):
            s = (r + amount) / r
            if not s > 0:
                raise ValueError(f"Deformation.radius: the radius {r} cannot change by {amount}")
            return (s, s, s if z else 1.0)

        return cls._scaling(surface, keep, (1 / r, 1 / r, z / r), factor)

    @classmethod
    def focus(cls, paraboloid, keep=None):
        from .g3d import shapes

        _, _, _, f = cls._leaf(paraboloid, (shapes.PARABOLOID,), "focus")

        def factor(amount):
            if not (f + amount) / f > 0:
                raise ValueError(f"Deformation.focus: the focus {f} cannot change by {amount}")
            s = np.sqrt((f + amount) / f)
            return (s, s, 1.0)

        return cls._scaling(paraboloid, keep, (1 / (2 * f), 1 / (2 * f), 0.0), factor)

    @classmethod
    def stretch(cls, part, axis, about=None):
        try:
            e = np.asarray(axis, dtype=float).reshape(-1)
        except (TypeError, ValueError):
            e = np.zeros(0)
        if e.shape != (3,) or not np.all(np.isfinite(e)) or not np.linalg.norm(e) > 0:
            raise ValueError(f"Deformation.stretch: axis is three finite numbers, not all zero (got {axis!r})")
        e = e / np.linalg.norm(e)
        out = cls(part, linear=np.outer(e, e), pivot=about)

        def finite(amount):
            if not 1 + amount > 0:
                raise ValueError(f"Deformation.stretch: a length cannot change by the factor {1 + amount}")
            m = np.eye(4)
            m[:3, :3] += amount * np.outer(e, e)
            m[:3, 3] = out.pivot - m[:3, :3] @ out.pivot
            return m

        out._finite = finite
        return out

    def generator(self):
        """The 4x4 matrix G with u(x) = G (x, 1)."""
        w = self.rotate
        g = np.zeros((4, 4))
        g[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + self.linear
        g[:3, 3] = self.translate - g[:3, :3] @ self.pivot
        return g

    def matrix(self, amount):
        amount = float(amount)
        if not np.isfinite(amount):
            raise ValueError("Deformation: amount is a finite number")
        return self._finite(amount) if self._finite is not None else _expm(amount * self.generator())

    def apply(self, amount):
        if not hasattr(self.part, "transform"):
            raise ValueError("Deformation.apply: the part was given as a bare id, there is nothing to transform")
        self.part.transform(self.matrix(amount))
        return self

    def __repr__(self):
        return (f"Deformation(surfaces={self.surface_ids}, translate={tuple(self.translate)}, rotate={tuple(self.rotate)}, "
                f"linear={self.linear.tolist()}, pivot={tuple(self.pivot)})")


class IndexChange:
    """One parameter of ``DeviceFrame.sensitivity``: the refractive index of the medium behind every leaf surface of
    ``part`` grows by ``rate`` per unit of the parameter, at every wavelength (the index following the wavelength by the
    glass's own dispersion is ``WavelengthChange``).  ``part``: an object with ``get_id()`` or a component, with a glass on at least one leaf."""

    def __init__(self, part, rate=1.0):
        from . import materials as matl

        if not hasattr(part, "surface_ids"):
            raise ValueError(f"IndexChange: part is a surface or a component (got {part!r})")
        leaves = list(part.surface_ids)
        if not any(isinstance(getattr(surface, "material", None), matl.Glass) for _, surface in leaves):
            raise ValueError("IndexChange: the part has no glass")
        if len({int(sid) for sid, _ in leaves}) > 64:
            raise ValueError(f"IndexChange: at most 64 surface ids a parameter (got {len(leaves)})")
        try:
            rate = float(rate)
        except (TypeError, ValueError):
            rate = np.nan
        if not np.isfinite(rate):
            raise ValueError("IndexChange: rate is a finite number")
        self.part, self.rate = part, rate
        self.surface_ids = tuple(sorted({int(sid) for sid, _ in leaves}))

    def __repr__(self):
        return f"IndexChange(surfaces={self.surface_ids}, rate={self.rate})"


def _ray_range(rays, what):
    """``rays`` of a SourceMotion or WavelengthChange as the id range [lo, hi) in floats: None is every ray."""
    if rays is None:
        return (-np.inf, np.inf)
    try:
        first, count = rays
        if first != int(first) or count != int(count) or isinstance(first, bool) or isinstance(count, bool):
            raise TypeError
        first, count = int(first), int(count)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what}: rays is None or (first_id, count), two integers (got {rays!r})") from None
    if first < 0 or count < 1 or first + count > 2 ** 53:
        raise ValueError(f"{what}: rays is None or (first_id, count) with first_id >= 0 and count >= 1 (got {rays!r})")
    return (float(first), float(first + count))


class SourceMotion:
    """One parameter of ``DeviceFrame.sensitivity``: a rigid motion of the launch of rays, per unit of the parameter.  The
    launch point o of a named ray moves with u = translate + rotate x (o - pivot), its unit direction with rotate x d
    (``translate``, ``rotate``, ``pivot`` as in ``Motion``; the pivot defaults to (0, 0, 0)).  ``rays``: None (every ray),
    ``(first_id, count)`` (the ids first_id .. first_id + count - 1) or ``SourceMotion.of_source(index, rays_per_source)``,
    which is ``(index * rays_per_source, rays_per_source)``, the tracer's own id rule; without ``rays_per_source`` the
    range is filled in by ``RayTracer.trace_sensitivity`` (its own) or by ``sensitivity(rays_per_source=)``.  It names
    no surfaces.  With two translations and two rotations the Jacobian and the slopes are the ray-transfer matrix about
    every real ray (``Sensitivity.transfer``)."""

    surface_ids = ()

    def __init__(self, rays=None, translate=(0.0, 0.0, 0.0), rotate=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0)):
        self.id_range = _ray_range(rays, "SourceMotion")
        self.rays = None if rays is None else (int(rays[0]), int(rays[1]))
        self.source = None
        vectors = []
        for name, value in (("translate", translate), ("rotate", rotate), ("pivot", pivot)):
            try:
                vector = np.asarray(value, dtype=float).reshape(-1)
            except (TypeError, ValueError):
                vector = np.zeros(0)
            if vector.shape != (3,) or not np.all(np.isfinite(vector)):
                raise ValueError(f"SourceMotion: {name} is three finite numbers (got {value!r})")
            vectors.append(vector)
        self.translate, self.rotate, self.pivot = vectors
        self.twist = np.concatenate(vectors)

    @classmethod
    def of_source(cls, index, rays_per_source=None, **motion):
        """The rays of source ``index``: ids [index * rays_per_source, (index + 1) * rays_per_source)."""
        try:
            if index != int(index) or isinstance(index, bool) or int(index) < 0:
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"SourceMotion.of_source: index is an integer >= 0 (got {index!r})") from None
        if rays_per_source is None:
            out = cls(None, **motion)
            out.id_range, out.source = None, int(index)
            return out
        try:
            if rays_per_source != int(rays_per_source) or isinstance(rays_per_source, bool) or int(rays_per_source) < 1:
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"SourceMotion.of_source: rays_per_source is an integer >= 1 (got {rays_per_source!r})") from None
        out = cls((int(index) * int(rays_per_source), int(rays_per_source)), **motion)
        out.source = int(index)
        return out

    def resolved(self, rays_per_source):
        """This parameter with its id range known: itself, or for ``of_source(index)`` a copy with ``rays_per_source``."""
        if self.id_range is not None:
            return self
        if not rays_per_source or rays_per_source is True:
            raise ValueError("sensitivity: SourceMotion.of_source(index) without rays_per_source needs "
                             "sensitivity(rays_per_source=) or RayTracer.trace_sensitivity")
        return SourceMotion.of_source(self.source, rays_per_source, translate=self.translate, rotate=self.rotate,
                                      pivot=self.pivot)

    def __repr__(self):
        rays = f"source {self.source}" if self.id_range is None else self.rays
        return (f"SourceMotion(rays={rays}, translate={tuple(self.translate)}, rotate={tuple(self.rotate)}, "
                f"pivot={tuple(self.pivot)})")


class WavelengthChange:
    """One parameter of ``DeviceFrame.sensitivity``: the wavelength of the named rays grows by ``rate`` micrometres per unit
    of the parameter.  The index behind every Sellmeier glass follows with that glass's own dn/dlambda at the ray's own
    wavelength (include/prt.h states the formula); a ``BasicRefractor`` has none, its rate is 0.  A table glass's
    ``index_at`` is host code without a derivative: ``sensitivity`` raises ``ValueError`` for a system that holds one.
    ``rays``: as in ``SourceMotion`` (None: every ray, or ``(first_id, count)``).  Known limit: a ray launched inside a
    glass keeps the index of its first segment."""

    surface_ids = ()

    def __init__(self, rays=None, rate=1.0):
        self.id_range = _ray_range(rays, "WavelengthChange")
        self.rays = None if rays is None else (int(rays[0]), int(rays[1]))
        try:
            rate = float(rate)
        except (TypeError, ValueError):
            rate = np.nan
        if not np.isfinite(rate):
            raise ValueError("WavelengthChange: rate is a finite number")
        self.rate = rate

    def __repr__(self):
        return f"WavelengthChange(rays={self.rays}, rate={self.rate})"


class Tolerances:
    """Manufacturing tolerances of the parameters of a ``sensitivity()`` call, one width per parameter, and the trials
    drawn from them.  ``distribution``: "uniform" on [-width, width]; "normal" with sigma = width (not truncated);
    "parabolic", the density 3 x^2 / (2 width^3) on [-width, width] that favours the ends of the range (a part made to
    the edge of its tolerance), variance 3 width^2 / 5.  ``sample(M)`` draws on the host from
    ``numpy.random.default_rng(seed)``: the same trials for the same seed, M and widths, call after call."""

    DISTRIBUTIONS = ("uniform", "normal", "parabolic")

    def __init__(self, widths, distribution="uniform", seed=0):
        try:
            w = np.asarray(widths, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            w = np.zeros(0)
        if not len(w) or not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError(f"widths: one finite number >= 0 per parameter (got {widths!r})")
        if distribution not in self.DISTRIBUTIONS:
            raise ValueError('distribution: "uniform", "normal" or "parabolic"')
        self.widths, self.distribution, self.seed = w, distribution, seed

    def sample(self, trials):
        """(trials, K) float64."""
        M = int(trials)
        if M != trials or M < 1:
            raise ValueError("trials: a whole number >= 1")
        rng = np.random.default_rng(self.seed)
        if self.distribution == "normal":
            unit = rng.standard_normal((M, len(self.widths)))
        else:
            unit = rng.uniform(-1.0, 1.0, (M, len(self.widths)))
            if self.distribution == "parabolic":
                unit = np.cbrt(unit)  # (the inverse of the distribution function (x^3 + 1) / 2)
        return unit * self.widths

    def sensitivity_table(self):
        """(2 K + 1, K): the nominal system, then per parameter k the trials 1 + 2 k (-width_k alone) and 2 + 2 k
        (+width_k alone): what ``ToleranceRun.table()`` reads."""
        K = len(self.widths)
        out = np.zeros((2 * K + 1, K))
        for k in range(K):
            out[1 + 2 * k, k], out[2 + 2 * k, k] = -self.widths[k], self.widths[k]
        return out


def moment_covariance(moments, n_columns):
    """The (C + 1, C + 1) longdouble covariance of (y_0 = OPD, y_1 .. y_C) from one group's block of
    ``prt_frame_tolerance_moments`` (rays kept, n_missed, n_unfollowed, sum w, sum w y_i, the lower triangle of
    sum w y_i y_j); None for a group without weight."""
    LD = np.longdouble
    wide = np.asarray(moments, dtype=LD)
    n = n_columns + 1
    sw = wide[3]
    if not sw > 0:
        return None
    mean = wide[4:4 + n] / sw
    lower = np.zeros((n, n), dtype=LD)
    lower[np.tril_indices(n)] = wide[4 + n:4 + n + n * (n + 1) // 2]
    second = (lower + np.tril(lower, -1).T) / sw
    return second - np.outer(mean, mean)


def _symmetric_pinv(matrix, rcond=None):
    """The pseudo-inverse of a symmetric positive semi-definite longdouble matrix (numpy.linalg stops at float64):
    equilibrated by its diagonal, diagonalised by cyclic Jacobi rotations, eigenvalues under ``rcond`` (default
    ``RANK_RCOND``) of the largest dropped.  Returns (pinv, rank)."""
    LD = np.longdouble
    rcond = RANK_RCOND if rcond is None else rcond
    a = np.array(matrix, dtype=LD)
    n = len(a)
    if not n:
        return a, 0
    scale = np.array([1 / np.sqrt(a[i, i]) if a[i, i] > 0 else LD(0) for i in range(n)], dtype=LD)
    a = a * scale[:, None] * scale[None, :]
    vectors = np.eye(n, dtype=LD)
    for _ in range(60):
        off = np.sqrt(np.sum(np.tril(a, -1) ** 2))
        if not off > np.finfo(LD).eps * max(np.sqrt(np.sum(np.diag(a) ** 2)), np.finfo(LD).tiny):
            break
        for i in range(n - 1):
            for j in range(i + 1, n):
                if a[i, j] == 0:
                    continue
                theta = (a[j, j] - a[i, i]) / (2 * a[i, j])
                t = np.sign(theta) / (abs(theta) + np.sqrt(theta * theta + 1)) if theta != 0 else LD(1)
                c = 1 / np.sqrt(t * t + 1)
                rot = np.eye(n, dtype=LD)
                rot[i, i] = rot[j, j] = c
                rot[i, j], rot[j, i] = t * c, -t * c
                a = rot.T @ a @ rot
                vectors = vectors @ rot
    values = np.diag(a)
    top = values.max() if n else LD(0)
    keep = values > rcond * top if top > 0 else np.zeros(n, dtype=bool)
    inverse = np.where(keep, 1 / np.where(keep, values, 1), 0)
    pinv = (vectors * inverse[None, :]) @ vectors.T
    return pinv * scale[:, None] * scale[None, :], int(keep.sum())


def solve_compensators(covariance, trials, free):
    """The coefficients of every column per trial, the columns ``free`` set to the least-squares minimiser of the
    variance of y_0 + sum_c q_c y_c.  ``covariance``: (C + 1, C + 1), of (y_0, y_1 .. y_C); ``trials``: (M, C), the
    drawn coefficients (what stands in a free column is overwritten); ``free``: column numbers in 0..C-1.  With A the
    free columns and N the others: q_A = -pinv(Cov_AA) (Cov_A0 + Cov_AN q_N), the minimum-norm one (in the columns
    scaled to unit variance) where Cov_AA is singular.  Returns (q (M, C) longdouble, rank); longdouble throughout."""
    LD = np.longdouble
    cov = np.asarray(covariance, dtype=LD)
    q = np.array(trials, dtype=LD)
    C = q.shape[1]
    free = np.asarray(sorted(free), dtype=np.int64)
    if not len(free):
        return q, 0
    fixed = np.setdiff1d(np.arange(C), free)
    pinv, rank = _symmetric_pinv(cov[np.ix_(1 + free, 1 + free)])
    rhs = cov[1 + free, 0][None, :] + q[:, fixed] @ cov[np.ix_(1 + fixed, 1 + free)]
    q[:, free] = -(rhs @ pinv.T)
    return q, rank


class ToleranceRun:
    """What ``Sensitivity.tolerance`` returns (numpy arrays), G groups, M trials, K parameters.  ``trials`` (M, K) as
    drawn; ``compensators`` and ``compensation`` (G, M, n_comp): what each compensator was set to, per trial and
    group -- for a real parameter the change ON TOP of the drawn value --; ``rms_opd`` (G, M): the RMS wavefront error
    of the trial after compensation, piston removed, in world units, from the quadratic form of the device's moments;
    ``strehl`` (G, M) and ``amplitude`` (G, L, M) complex: the Strehl ratio and U_l of include/prt.h
    (``prt_frame_tolerance``), the merit fully nonlinear in the moved OPDs; ``rms_radius`` (G, M): the RMS spot radius
    from the landing points' quadratic (``Sensitivity.mean_square``, its gradient and ``normal_matrix``) at the
    compensated real parameters -- NaN throughout when "focus" is a compensator, since a focus shift moves a landing
    point along its ray and that needs the slopes; "tilt" moves the evaluation point only and leaves the radius about
    the centroid alone --; ``nominal``: the all-zero trial with the same compensators (``strehl``, ``rms_opd``,
    ``rms_radius`` (G) and ``compensation`` (G, n_comp)); per group and wavelength ``n_rays``, ``n_missed``,
    ``n_unfollowed``; ``record`` the device's (G, L, 5) block; ``moments`` its (G, ...) moments block."""

    def __init__(self, trials, compensators, compensation, rms_opd, strehl, amplitude, rms_radius, record, moments,
                 wavelengths, world_unit_um, parameters, follow):
        self.compensators = tuple(compensators)
        self.trials = np.asarray(trials, dtype=float)[:-1]
        self.compensation, self.rms_opd, self.strehl = compensation[:, :-1], rms_opd[:, :-1], strehl[:, :-1]
        self.amplitude, self.rms_radius = amplitude[:, :, :-1], rms_radius[:, :-1]
        self.nominal = SimpleNamespace(compensation=compensation[:, -1], rms_opd=rms_opd[:, -1], strehl=strehl[:, -1],
                                       rms_radius=rms_radius[:, -1], amplitude=amplitude[:, :, -1])
        self.record, self.moments = np.asarray(record, dtype=float), np.asarray(moments, dtype=float)
        self.n_rays, self.n_missed, self.n_unfollowed = (self.record[:, :, k].astype(np.int64) for k in (0, 1, 2))
        self.wavelengths, self.world_unit_um = np.asarray(wavelengths, dtype=float), world_unit_um
        self.parameters, self.follow = tuple(parameters), follow
        self.n_parameters, self.n_trials = len(self.parameters), len(self.trials)

    def yield_(self, strehl=0.8):
        """(G): the share of the trials whose Strehl ratio is at least ``strehl``; NaN for a group without rays."""
        with np.errstate(invalid="ignore"):
            passed = np.mean(self.strehl >= strehl, axis=1)
        return np.where(np.all(np.isfinite(self.strehl), axis=1), passed, np.nan)

    def percentiles(self, q=(2, 10, 50, 90, 98)):
        """Per merit a (G, len(q)) array of its percentiles over the trials: ``strehl``, ``rms_opd``, ``rms_radius``."""
        q = np.atleast_1d(np.asarray(q, dtype=float))
        with np.errstate(invalid="ignore"):
            return {name: np.percentile(getattr(self, name), q, axis=1).T for name in ("strehl", "rms_opd", "rms_radius")}

    def to_pandas(self):
        """One row per (group, trial): the merits, the drawn parameters ``p_k`` and the compensation ``c_<name>``."""
        G, M = self.strehl.shape
        data = {"source_id": np.repeat(np.arange(G), M), "trial": np.tile(np.arange(M), G),
                "strehl": self.strehl.ravel(), "rms_opd": self.rms_opd.ravel(), "rms_radius": self.rms_radius.ravel()}
        for k in range(self.n_parameters):
            data[f"p_{k}"] = np.tile(self.trials[:, k], G)
        for j, name in enumerate(self._compensator_names()):
            data[f"c_{name}"] = self.compensation[:, :, j].ravel()
        return pd.DataFrame(data)

    def _compensator_names(self):
        names = []
        for c in self.compensators:
            names += ["tilt_u", "tilt_v"] if c == "tilt" else [str(c)]
        return names

    def table(self, group=0):
        """For a run on ``Tolerances.sensitivity_table()``: per parameter the change of each merit against the nominal
        trial at -width and +width (``dstrehl_minus``, ``dstrehl_plus``, ``drms_opd_*``, ``drms_radius_*``) and
        ``worst``, the lower of the two Strehl changes; the rows sorted worst first.  ``ValueError`` for other trials."""
        K = self.n_parameters
        t = self.trials
        one_at_a_time = t.shape == (2 * K + 1, K) and not np.any(t[0])
        for k in range(K if one_at_a_time else 0):
            hot = np.zeros(K, dtype=bool)
            hot[k] = True
            one_at_a_time &= (not np.any(t[1 + 2 * k][~hot]) and not np.any(t[2 + 2 * k][~hot])
                              and t[1 + 2 * k, k] == -t[2 + 2 * k, k])
        if not one_at_a_time:
            raise ValueError("table: the trials are not Tolerances.sensitivity_table()'s")
        rows = {"parameter": np.arange(K), "width": t[2::2][np.arange(K), np.arange(K)]}
        for name in ("strehl", "rms_opd", "rms_radius"):
            merit = getattr(self, name)[group]
            rows[f"d{name}_minus"], rows[f"d{name}_plus"] = merit[1::2] - merit[0], merit[2::2] - merit[0]
        rows["worst"] = np.fmin(rows["dstrehl_minus"], rows["dstrehl_plus"])
        return pd.DataFrame(rows).sort_values("worst", kind="stable").reset_index(drop=True)


class _TrialMoments:
    """What ``MTFToleranceRun`` and ``EnergyToleranceRun`` read from the device's moments (G, M + 1, 8) and record, in
    longdouble on the host: the two passes hand over the same block, so they share this arithmetic."""

    def _read_moments(self, moments, record, focus_shift, focus):
        """Sets ``focus``, ``moments``, ``record`` and the per-group fields; returns the whole (G, M + 1, ...) arrays
        ``focus_shift``, ``centroid``, ``rms_radius`` and ``best_focus``, the nominal trial last."""
        LD = np.longdouble
        self.focus = np.asarray(focus, dtype=float)
        self.moments, self.record = np.asarray(moments, dtype=float), np.asarray(record, dtype=float)
        self.centre, self.sum_weights = self.record[:, :3], self.record[:, 3]
        self.n_rays, self.n_missed, self.n_unfollowed = (np.nan_to_num(self.record[:, k]).astype(np.int64) for k in (4, 5, 6))
        shift = np.asarray(focus_shift, dtype=float)
        wide = self.moments.astype(LD)
        with np.errstate(invalid="ignore", divide="ignore"):
            sw = np.where(wide[..., 0] > 0, wide[..., 0], np.nan)
            mean_p, mean_s = wide[..., 1:3] / sw[..., None], wide[..., 3:5] / sw[..., None]
            var_p = wide[..., 5] / sw - np.sum(mean_p * mean_p, axis=-1)
            cov = wide[..., 6] / sw - np.sum(mean_p * mean_s, axis=-1)
            var_s = wide[..., 7] / sw - np.sum(mean_s * mean_s, axis=-1)
            best = np.where(var_s > 0, -cov / np.where(var_s > 0, var_s, 1), np.where(np.isnan(sw), np.nan, 0))
            planes = self.focus.astype(LD)[None, None, :] + shift.astype(LD)[:, :, None]  # (G, M, F)
            self._mean_p, self._mean_s, self._planes = mean_p, mean_s, planes
            square = var_p[..., None] + 2 * planes * cov[..., None] + planes * planes * var_s[..., None]
            rms_radius = np.sqrt(np.maximum(square, 0)).astype(float)
        return dict(focus_shift=shift, centroid=self.centroid_at(0), rms_radius=rms_radius, best_focus=best.astype(float))

    def centroid_at(self, plane):
        """(G, M + 1, 2): every trial's centroid (the nominal trial last) in the plane ``focus[plane] + focus_shift``."""
        return (self._mean_p + self._planes[:, :, plane, None] * self._mean_s).astype(float)

    def _one_at_a_time(self):
        """K, for a run on ``Tolerances.sensitivity_table()``'s trials; ``ValueError`` for other trials."""
        K = self.n_parameters
        t = self.trials
        one_at_a_time = t.shape == (2 * K + 1, K) and not np.any(t[0])
        for k in range(K if one_at_a_time else 0):
            hot = np.zeros(K, dtype=bool)
            hot[k] = True
            one_at_a_time &= (not np.any(t[1 + 2 * k][~hot]) and not np.any(t[2 + 2 * k][~hot])
                              and t[1 + 2 * k, k] == -t[2 + 2 * k, k])
        if not one_at_a_time:
            raise ValueError("table: the trials are not Tolerances.sensitivity_table()'s")
        return K


class MTFToleranceRun(_TrialMoments):
    """What ``Sensitivity.mtf_tolerance`` returns (numpy arrays), G groups, M trials, K parameters, F focus shifts, A
    azimuths, N frequencies.  ``trials`` (M, K) as drawn; ``otf`` (G, M, F, A, N) complex and ``mtf`` = |otf|: the
    geometric OTF of every trial under the linear ray model, the merit fully nonlinear in the moved landing points
    (``prt_frame_mtf_tolerance``; include/prt.h states the formulas), at the planes ``focus[f] + focus_shift``;
    ``focus_shift`` (G, M): the plane shift the trial was evaluated at on top of ``focus`` -- the device's least-squares
    refocus with the "focus" compensator, zeros without --; ``best_focus`` (G, M): the least-squares focus
    -cov(P, S) / var(S) of the trial from its moments, whether compensated or not (0 where var(S) is not > 0);
    ``rms_radius`` (G, M, F): the RMS spot radius about the trial's own centroid in each of those planes, and
    ``centroid`` (G, M, 2): that centroid in the first plane, ``focus[0] + focus_shift``, as (e1, e2) coordinates about
    the centre C_g (``centroid_at(plane)`` for another) -- both from the device's moments, in longdouble on the host.
    ``reference``: "fixed", the kernel's numbers about the held centre, or "centroid", each trial's OTF about its own
    centroid, what ``frame.mtf()`` of the perturbed system reports; ``mtf`` is the same under both.  ``nominal``: the
    same fields for the all-zero trial.  Per group ``centre`` (G, 3), ``sum_weights``, ``n_rays``, ``n_missed``,
    ``n_unfollowed``; ``moments`` the device's (G, M + 1, 8) block (sum w, sum w P (2), sum w S (2), sum w P.P,
    sum w P.S, sum w S.S; the nominal trial last), ``record`` its (G, 7) block.  A group without rays is NaN."""

    FIELDS = ("otf", "mtf", "focus_shift", "centroid", "rms_radius", "best_focus")

    def __init__(self, trials, otf, moments, focus_shift, record, frequencies, azimuths, focus, parameters,
                 compensators=(), reference="fixed"):
        self.frequencies = np.asarray(frequencies, dtype=float)
        self.azimuths = np.asarray(azimuths, dtype=float)
        self.parameters, self.compensators, self.reference = tuple(parameters), tuple(compensators), reference
        whole = self._read_moments(moments, record, focus_shift, focus)
        mean_p, mean_s, planes = self._mean_p, self._mean_s, self._planes
        otf = np.asarray(otf)
        if reference == "centroid":  # (about each trial's own centroid in each plane: the phase of the shift back)
            angle = np.radians(self.azimuths)
            kc, ks = np.cos(angle)[:, None] * self.frequencies, np.sin(angle)[:, None] * self.frequencies  # (A, N)
            with np.errstate(invalid="ignore"):
                c = (mean_p[:, :, None, :] + planes[..., None] * mean_s[:, :, None, :]).astype(float)  # (G, M, F, 2)
            otf = otf * np.exp(2j * np.pi * (c[..., 0, None, None] * kc + c[..., 1, None, None] * ks))
        whole = dict(otf=otf, mtf=np.abs(otf), **whole)
        for name, value in whole.items():
            setattr(self, name, value[:, :-1])
        self.nominal = SimpleNamespace(**{name: value[:, -1] for name, value in whole.items()})
        self.trials = np.asarray(trials, dtype=float)[:-1]
        self.n_parameters, self.n_trials = len(self.parameters), len(self.trials)

    def _outputs(self, frequency, azimuth, plane):
        """``mtf`` (G, M, ...) cut to the selected plane (an index), azimuths and frequencies (indices, or None: all)."""
        cut = self.mtf[:, :, plane]
        cut = cut if azimuth is None else cut[:, :, np.atleast_1d(azimuth)]
        return cut if frequency is None else cut[:, :, :, np.atleast_1d(frequency)]

    def yield_(self, threshold, frequency=None, azimuth=None, plane=0):
        """(G): the share of the trials whose MTF is at least ``threshold`` at every selected output of the plane
        ``plane``; ``frequency`` and ``azimuth`` are indices (or lists of them), None for all; NaN for a group
        without rays."""
        cut = self._outputs(frequency, azimuth, plane)
        cut = cut.reshape(cut.shape[0], cut.shape[1], -1)
        with np.errstate(invalid="ignore"):
            passed = np.mean(np.all(cut >= threshold, axis=2), axis=1)
        return np.where(np.all(np.isfinite(cut), axis=(1, 2)), passed, np.nan)

    def percentiles(self, q=(2, 10, 50, 90, 98), frequency=-1, azimuth=0, plane=0):
        """(G, len(q)): the percentiles over the trials of the MTF at one output (indices)."""
        q = np.atleast_1d(np.asarray(q, dtype=float))
        with np.errstate(invalid="ignore"):
            return np.percentile(self.mtf[:, :, plane, azimuth, frequency], q, axis=1).T

    def to_pandas(self):
        """One row per (group, trial): ``focus_shift``, ``best_focus``, per plane ``rms_radius_<f>``, per output
        ``mtf_<f>_<a>_<n>`` (indices of plane, azimuth, frequency) and the drawn parameters ``p_k``."""
        G, M = self.focus_shift.shape
        data = {"source_id": np.repeat(np.arange(G), M), "trial": np.tile(np.arange(M), G),
                "focus_shift": self.focus_shift.ravel(), "best_focus": self.best_focus.ravel()}
        for f in range(len(self.focus)):
            data[f"rms_radius_{f}"] = self.rms_radius[:, :, f].ravel()
        for f in range(len(self.focus)):
            for a in range(len(self.azimuths)):
                for n in range(len(self.frequencies)):
                    data[f"mtf_{f}_{a}_{n}"] = self.mtf[:, :, f, a, n].ravel()
        for k in range(self.n_parameters):
            data[f"p_{k}"] = np.tile(self.trials[:, k], G)
        return pd.DataFrame(data)

    def table(self, group=0, frequency=-1, plane=0):
        """For a run on ``Tolerances.sensitivity_table()``: per parameter the change of the MTF at one frequency and
        plane (indices) against the nominal trial at -width and +width, each the worst (lowest) over the azimuths
        (``dmtf_minus``, ``dmtf_plus``), and ``worst``, the lower of the two; the rows sorted worst first.
        ``ValueError`` for other trials."""
        K, t = self._one_at_a_time(), self.trials
        merit = self.mtf[group, :, plane, :, frequency]  # (M, A)
        change = (merit[1:] - merit[0]).min(axis=1)
        rows = {"parameter": np.arange(K), "width": t[2::2][np.arange(K), np.arange(K)], "dmtf_minus": change[0::2],
                "dmtf_plus": change[1::2]}
        rows["worst"] = np.fmin(rows["dmtf_minus"], rows["dmtf_plus"])
        return pd.DataFrame(rows).sort_values("worst", kind="stable").reset_index(drop=True)


class EnergyToleranceRun(_TrialMoments):
    """What ``Sensitivity.energy_tolerance`` returns (numpy arrays), G groups, M trials, K parameters, F focus shifts, R
    radii, N fractions.  ``trials`` (M, K) as drawn; ``energy`` (G, M, F, R): the share of the energy within each of
    ``radii`` of every trial under the linear ray model, the merit fully nonlinear in the moved landing points, and
    ``count`` (G, M, F, R) uint64, the exact integer count it is the quotient of (``energy = count / total``);
    ``radius`` (G, M, F, N): the radius (half-width for a square or a slit) that holds each of ``fractions``, a ray's own
    distance (the pass of include/prt.h under the energy tolerancing; it states the formulas) -- all at the planes
    ``focus[f] + focus_shift``, about the trial's own centroid there (``follow_centroid``) or about the held centre.
    ``focus_shift`` (G, M), ``best_focus`` (G, M), ``rms_radius`` (G, M, F), ``centroid`` (G, M, 2) and
    ``centroid_at(plane)`` from the device's moments, as in ``MTFToleranceRun``.  ``nominal``: the same fields for the
    all-zero trial.  Per group ``total`` (uint64: W, the sum of the integer weights), ``centre`` (G, 3), ``sum_weights``,
    ``n_rays``, ``n_missed``, ``n_unfollowed``; ``moments`` the device's (G, M + 1, 8) block (the nominal trial last),
    ``record`` its (G, 7) block, both with the bits ``mtf_tolerance`` gives.  A group without rays, or without weight,
    is NaN, its counts 0."""

    FIELDS = ("energy", "count", "radius", "focus_shift", "centroid", "rms_radius", "best_focus")

    def __init__(self, trials, count, energy, radius, moments, focus_shift, record, radii, fractions, focus, parameters,
                 shape="circle", compensators=(), follow_centroid=True):
        self.radii, self.fractions = np.asarray(radii, dtype=float), np.asarray(fractions, dtype=float)
        self.parameters, self.compensators = tuple(parameters), tuple(compensators)
        self.shape, self.follow_centroid = shape, bool(follow_centroid)
        record = np.ascontiguousarray(record, dtype=np.float64)
        self.total = record[:, 7].copy().view(np.uint64)  # (the device hands W over as its bit image)
        whole = self._read_moments(moments, record[:, :7], focus_shift, focus)
        whole = dict(energy=np.asarray(energy, dtype=float), count=np.asarray(count).astype(np.uint64, copy=False),
                     radius=np.asarray(radius, dtype=float), **whole)
        for name, value in whole.items():
            setattr(self, name, value[:, :-1])
        self.nominal = SimpleNamespace(**{name: value[:, -1] for name, value in whole.items()})
        self.trials = np.asarray(trials, dtype=float)[:-1]
        self.n_parameters, self.n_trials = len(self.parameters), len(self.trials)

    @staticmethod
    def _share(cut, passed):
        """(G): the mean of ``passed`` (G, M) over the trials, NaN for a group whose ``cut`` (G, M) is not finite."""
        return np.where(np.all(np.isfinite(cut), axis=1), np.mean(passed, axis=1), np.nan)

    def yield_(self, fraction_at_least, radius=0, plane=0):
        """(G): the share of the trials that put at least ``fraction_at_least`` of the energy within ``radii[radius]``
        in the plane ``plane`` (indices); NaN for a group without rays."""
        cut = self.energy[:, :, plane, radius]
        with np.errstate(invalid="ignore"):
            return self._share(cut, cut >= fraction_at_least)

    def yield_radius(self, at_most, fraction=-1, plane=0):
        """(G): the share of the trials whose radius of ``fractions[fraction]`` is at most ``at_most`` in the plane
        ``plane`` (indices); NaN for a group without rays."""
        cut = self.radius[:, :, plane, fraction]
        with np.errstate(invalid="ignore"):
            return self._share(cut, cut <= at_most)

    def percentiles(self, q=(2, 10, 50, 90, 98), fraction=-1, plane=0):
        """(G, len(q)): the percentiles over the trials of the radius of one fraction in one plane (indices)."""
        q = np.atleast_1d(np.asarray(q, dtype=float))
        with np.errstate(invalid="ignore"):
            return np.percentile(self.radius[:, :, plane, fraction], q, axis=1).T

    def to_pandas(self):
        """One row per (group, trial): ``focus_shift``, ``best_focus``, per plane ``rms_radius_<f>``, per output
        ``energy_<f>_<j>`` and ``radius_<f>_<k>`` (indices of plane, radius, fraction) and the drawn parameters
        ``p_k``."""
        G, M = self.focus_shift.shape
        data = {"source_id": np.repeat(np.arange(G), M), "trial": np.tile(np.arange(M), G),
                "focus_shift": self.focus_shift.ravel(), "best_focus": self.best_focus.ravel()}
        for f in range(len(self.focus)):
            data[f"rms_radius_{f}"] = self.rms_radius[:, :, f].ravel()
        for f in range(len(self.focus)):
            for j in range(len(self.radii)):
                data[f"energy_{f}_{j}"] = self.energy[:, :, f, j].ravel()
            for k in range(len(self.fractions)):
                data[f"radius_{f}_{k}"] = self.radius[:, :, f, k].ravel()
        for k in range(self.n_parameters):
            data[f"p_{k}"] = np.tile(self.trials[:, k], G)
        return pd.DataFrame(data)

    def table(self, group=0, fraction=-1, plane=0):
        """For a run on ``Tolerances.sensitivity_table()``: per parameter the change of the radius of one fraction in
        one plane (indices) against the nominal trial at -width and +width (``dradius_minus``, ``dradius_plus``), and
        ``worst``, the larger of the two; the rows sorted worst (largest growth of the radius) first.  ``ValueError``
        for other trials."""
        K, t = self._one_at_a_time(), self.trials
        merit = self.radius[group, :, plane, fraction]  # (M)
        change = merit[1:] - merit[0]
        rows = {"parameter": np.arange(K), "width": t[2::2][np.arange(K), np.arange(K)], "dradius_minus": change[0::2],
                "dradius_plus": change[1::2]}
        rows["worst"] = np.fmax(rows["dradius_minus"], rows["dradius_plus"])
        return pd.DataFrame(rows).sort_values("worst", ascending=False, kind="stable").reset_index(drop=True)


class Sensitivity:
    """What ``DeviceFrame.sensitivity`` found.  ``jacobian``: device (K, 3, n_selected) float64, d(x1, y1, z1)/dp_k of the
    selected rows, which ``rows()`` names (frame row numbers, ordered by group, generation and id); NaN for a ray that
    could not be followed.  Per group, from the device's sums (``sums``, the layout of include/prt.h): ``weight``,
    ``centroid``, ``mean_square`` (radius about the centroid, or about the fixed ``reference``), ``centroid_gradient``
    (groups, K, 3), ``mean_square_gradient`` and ``rms_radius_gradient`` (groups, K), ``normal_matrix`` (groups, K, K) and
    ``rhs`` (groups, K) of the Gauss-Newton step that ``step()`` solves.  A group without rows has NaN there.
    ``n_unknown`` / ``n_invalid`` / ``n_unfit``: rays lost to a surface that ``system`` does not hold, to a row that is
    not finite, to an interface whose rows fit no rule; ``n_reflections``: reflections differentiated.

    With a ``SourceMotion`` or a ``WavelengthChange`` among the parameters also ``slopes``: device (K, 3, n_selected)
    float64, the derivative of the selected rows' unit directions, NaN where ``jacobian`` is; on top of both
    ``focus_gradient()``, ``transfer()`` and ``effective_focal_length()``; so also with ``sensitivity(slopes=True)``,
    whatever the parameters are, and then ``mtf_gradient()`` gives d(OTF)/d(parameter) through focus.  ``slopes`` is None
    otherwise.

    With ``sensitivity(wavefront=)`` also, against that ``Wavefront``'s reference sphere held fixed (device tensors in the
    order of ``rows()``, NaN for a ray that misses the sphere or could not be followed): ``dfield`` (K, n_selected), the
    change of the wavefront at a fixed pupil point; ``dopd`` (K, n_selected), the derivative of the ray's own OPD, following
    the ray; ``dpupil`` (K, 2, n_selected), the motion of its normalised pupil point; ``opd`` and ``pupil``, the row's OPD
    about the pivot and its pupil point as the pass evaluated them.  Per group: ``opd_sums`` (the layout of include/prt.h),
    ``n_missed``, ``dzernike()``, ``wavefront_variance_gradient`` and ``rms_opd_gradient`` (groups, K): the exact
    derivatives of the sample statistic that ``Wavefront.rms`` reports (from ``dopd``, piston removed), over the rays
    that were followed; ``psf_gradient()`` gives d(PSF) and d(Strehl)/d(parameter) of the diffraction image.
    ``wavefront`` is the Wavefront; None, and none of these, without the argument."""

    def __init__(self, jacobian, selected, sums, pivots, centred, record, parameters, wave=None, launch=None):
        self.slopes = None if launch is None else launch["slopes"]
        self._launch = launch
        self.jacobian, self._selected, self.sums, self.pivots, self.centred = jacobian, selected, sums, pivots, centred
        self.parameters = tuple(parameters)
        self.n_unknown, self.n_invalid, self.n_unfit, self.n_reflections = (int(v) for v in record)
        K = self.n_parameters = len(self.parameters)
        wide = np.asarray(sums, dtype=np.longdouble)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.count = np.asarray(sums[:, 0], dtype=np.int64)
            sw = np.where(wide[:, 1] > 0, wide[:, 1], np.nan)
            offset = wide[:, 2:5] / sw[:, None] - pivots  # (centroid - pivot)
            sq = wide[:, 5] / sw
            sd = wide[:, 6:6 + 3 * K].reshape(-1, K, 3)
            sxd = wide[:, 6 + 3 * K:6 + 4 * K]
            lower = np.zeros((len(wide), K, K), dtype=np.longdouble)
            tri = np.tril_indices(K)
            lower[:, tri[0], tri[1]] = wide[:, 6 + 4 * K:]
            moments = lower + np.transpose(np.tril(lower, -1), (0, 2, 1))
            if centred:
                sq = sq - np.sum(offset * offset, axis=1)
                sxd = sxd - np.einsum("gc,gkc->gk", offset, sd)
                moments = moments - np.einsum("gjc,gkc->gjk", sd, sd) / sw[:, None, None]
            self.weight = np.asarray(sw, dtype=float)
            self.centroid = np.asarray(offset + pivots, dtype=float)
            self.mean_square = np.asarray(sq, dtype=float)
            self.centroid_gradient = np.asarray(sd / sw[:, None, None], dtype=float)
            self.mean_square_gradient = np.asarray(2 * sxd / sw[:, None], dtype=float)
            self.rms_radius_gradient = self.mean_square_gradient / (2 * np.sqrt(self.mean_square))[:, None]
            self.normal_matrix = np.asarray(moments / sw[:, None, None], dtype=float)
            self.rhs = -self.mean_square_gradient / 2
        self.wavefront = None
        if wave is not None:
            self._wave(wave)

    def _wave(self, wave):
        """The per-group wavefront results from the device's sums, in longdouble as the others are."""
        self.wavefront = wave["wavefront"]
        self.dfield, self.dopd, self.dpupil, self.opd, self.pupil = (wave[k] for k in ("dfield", "dopd", "dpupil", "opd", "pupil"))
        self.opd_sums = wave["sums"]
        K, J = self.n_parameters, self.wavefront.terms
        wide = np.asarray(self.opd_sums, dtype=np.longdouble)
        self.n_missed = np.asarray(self.opd_sums[:, 1], dtype=np.int64)
        at = 5 + J * (K + 3)
        with np.errstate(invalid="ignore", divide="ignore"):
            sw = np.where(wide[:, 2] > 0, wide[:, 2], np.nan)[:, None]
            mean = wide[:, 3:4] / sw
            variance = wide[:, 4:5] / sw - mean * mean
            self._z_rhs = np.asarray(wide[:, 5:at].reshape(-1, K + 3, J), dtype=float)  # (columns dfield_k, then n u_c)
            dopd, opd_dopd, dfield, opd_dfield = (wide[:, at + q * K:at + (q + 1) * K] / sw for q in range(4))
            lower = np.zeros((len(wide), K, K), dtype=np.longdouble)
            tri = np.tril_indices(K)
            lower[:, tri[0], tri[1]] = wide[:, at + 4 * K:]
            moments = (lower + np.transpose(np.tril(lower, -1), (0, 2, 1))) / sw[:, :, None]
            self.wavefront_variance = np.asarray(variance[:, 0], dtype=float)
            self.wavefront_variance_gradient = np.asarray(2 * (opd_dopd - mean * dopd), dtype=float)
            self.rms_opd_gradient = self.wavefront_variance_gradient / (2 * np.sqrt(self.wavefront_variance))[:, None]
            # Gauss-Newton on the piston-removed OPD, dfield the Jacobian: both centred on their weighted means
            self._wave_weight = np.asarray(sw[:, 0], dtype=float)
            self.wavefront_normal_matrix = np.asarray(moments - dfield[:, :, None] * dfield[:, None, :], dtype=float)
            self.wavefront_rhs = np.asarray(-(opd_dfield - mean * dfield), dtype=float)

    def _need_wave(self, what):
        if self.wavefront is None:
            raise ValueError(f"{what}: this Sensitivity was made without sensitivity(wavefront=)")

    def dzernike(self, reference="fixed"):
        """(groups, K, J): per parameter the Zernike expansion of the wavefront change ``dfield_k``, the least-squares fit
        through ``solve_normal_equations`` with the Wavefront's own ``Z^T W Z`` at the rows' nominal pupil points.
        ``reference="fixed"``: the reference sphere stays where it is.  ``"centroid"``: its centre follows the group's
        centroid, ``dfield_k - n (u.dP_k)`` with ``dP_k`` this object's ``centroid_gradient`` (the weighted centroid of the
        rays that were followed: the Wavefront's own "centroid" where the weights are equal); R stays.

        This is the expansion of the wavefront CHANGE.  It equals the derivative of the fitted coefficients
        ``Wavefront.zernike`` exactly where the residual of that fit is zero; elsewhere it leaves out the terms that come
        from the sample points moving in the pupil (``dZ/dp`` at ``dpupil``, times the residual), which vanish as the
        sampling of the pupil gets dense.  Rays that were not followed have no part in the right-hand sides while they
        have one in ``Z^T W Z``."""
        self._need_wave("dzernike")
        if reference not in ("fixed", "centroid"):
            raise ValueError('reference: "fixed" or "centroid"')
        K, J = self.n_parameters, self.wavefront.terms
        rhs = self._z_rhs[:, :K, :]
        if reference == "centroid":
            rhs = rhs - np.einsum("gkc,gcj->gkj", self.centroid_gradient, self._z_rhs[:, K:, :])
        tri = J * (J + 1) // 2
        out = np.full((len(rhs), K, J), np.nan)
        for k in range(K):
            packed = np.array(self.wavefront.normal, dtype=float)
            usable = np.all(np.isfinite(rhs[:, k, :]), axis=1)
            packed[:, tri:tri + J] = np.where(usable[:, None], rhs[:, k, :], 0.0)
            packed[~usable, -3] = 0.0
            out[:, k, :] = solve_normal_equations(packed, J)[0]
        return out

    def _selected_rows(self):
        """The nine leading arguments of the passes over the selected rows (``mtf_gradient``, ``psf_gradient``,
        ``tolerance``): the frame's rows, the selection in its order, where every group begins, the weights' column."""
        rows, weights, first = (self._launch[k] for k in ("rows", "weights", "group_first"))
        first = np.ascontiguousarray(first, dtype=np.int64)
        return _SelectedRows(*_row_head(rows), self._selected, int(self._selected.shape[0]), first, len(first) - 1,
                             _weight_column(weights))

    def _wavelengths_for(self, what, follow, closing):
        """What ``psf_gradient`` and ``tolerance`` (``what``) check before they allocate: ``follow``, no
        ``WavelengthChange`` among the parameters (``closing`` ends the caller's sentence), a frame recorded with its
        wavelengths and a selection that is not empty.  Returns the distinct wavelengths of the selected rows."""
        if follow not in ("ray", "pupil"):
            raise ValueError('follow: "ray" or "pupil"')
        if any(isinstance(m, WavelengthChange) for m in self.parameters):
            raise ValueError(f"{what}: a WavelengthChange among the parameters moves a ray between wavelengths; {closing}")
        written = self._launch.get("written")
        if written is not None and _INDEX["wavelength"] not in written:
            raise ValueError(f"{what}: the frame was recorded without the wavelength column (RecordPlan(columns=...))")
        if not len(self._selected):
            raise ValueError(f"{what}: no row is selected at this surface")
        wavelength = self._launch["rows"][_INDEX["wavelength"]][self._selected]
        return _distinct_wavelengths(wavelength.unique().cpu().numpy().astype(np.float64), what)

    def _need_slopes(self, what):
        if self.slopes is None:
            raise ValueError(f"{what}: this Sensitivity has no slopes (they come with sensitivity(slopes=True), or with a "
                             "SourceMotion or a WavelengthChange among the parameters)")

    def mtf_gradient(self, frequencies, *, azimuths=(0.0, 90.0), focus=(0.0,), reference="fixed", centre=None, axis=None,
                     basis=None):
        """d(OTF)/d(parameter) of the geometric MTF of the selected rows, per group, at every focus shift, azimuth and
        frequency, from this one trace: an ``MTFGradient``.  Needs ``slopes`` (``sensitivity(slopes=True)``): the MTF is
        taken through focus, on planes a ray reaches as a straight line, so the derivative of its direction enters.

        ``frequencies``, ``azimuths``, ``focus``, ``axis`` and ``basis`` as in ``DeviceFrame.mtf``; the weights are the
        ``sensitivity()`` call's.  A ray is summed if ``mtf()`` would keep it and its ``jacobian`` and ``slopes`` are
        finite for every parameter -- one set of rays for all parameters; the others are counted (``n_missed``,
        ``n_unfollowed``) and contribute nothing.  ``centre``: None for the weighted centroid of the rays summed, or a
        point, or a (groups, 3) array.  ``reference="fixed"``: the centre is held fixed under the parameter, the
        kernel's own numbers (``prt_frame_mtf_gradient``; include/prt.h states the formulas).  ``"centroid"``: the
        centre follows the group's centroid, composed on the host as
        ``dotf_k + 2 pi i (k.(dC_k.e1, dC_k.e2)) otf + (dC_k.a) dotf_dfocus`` -- |OTF|, and so ``dmtf``, is the same
        under both; the phase is not.  The result is the derivative at fixed path, as ``jacobian`` is."""
        self._need_slopes("mtf_gradient")
        import torch

        from . import engine

        if reference not in ("fixed", "centroid"):
            raise ValueError('reference: "fixed" or "centroid"')
        nu, theta, planes = _mtf_sampling(frequencies, azimuths, focus)
        axes = pupil_axes(axis, basis)
        head = self._selected_rows()
        dev, n_selected, n_groups, K = head.rows.device, head.n_selected, head.n_groups, self.n_parameters
        centres = None if centre is None else _group_points(centre, n_groups, dev, "centre: None, a point")
        shape = (len(planes), len(theta), len(nu))
        otf = torch.empty((n_groups,) + shape + (2,), dtype=torch.float64, device=dev)
        dotf = torch.empty((n_groups, K + 1) + shape + (2,), dtype=torch.float64, device=dev)
        record = torch.empty((n_groups, 7 + 3 * K), dtype=torch.float64, device=dev)
        engine.call("prt_frame_mtf_gradient", *head, self.jacobian.contiguous(), self.slopes.contiguous(), K, centres, axes,
                    nu, len(nu), theta, len(theta), planes, len(planes), otf, dotf, record, device=dev,
                    size=(n_selected, n_groups, K, len(nu), len(theta), len(planes)))
        return MTFGradient(engine.host_complex(otf), engine.host_complex(dotf), engine.host(record), nu, theta, planes, axes,
                           self.parameters, reference)

    def psf_gradient(self, *, world_unit_um, pixels=64, pixel_size=None, centre=(0.0, 0.0), follow="ray"):
        """d(PSF)/d(parameter) and d(Strehl)/d(parameter) of the diffraction image of the selected rows, per group, from
        this one trace: a ``PSFGradient``.  Needs ``sensitivity(wavefront=)``: the rays, their OPD and pupil points, the
        reference sphere (held fixed) and the weights are that call's; ``world_unit_um``, ``pixels``, ``pixel_size`` (default
        lambda_min * F / 4) and ``centre`` as in ``DeviceFrame.psf``.  One HIP pass (``prt_frame_psf_gradient``;
        include/prt.h states the formulas): the Huygens sum of ``psf()`` with, per parameter, the derivative of every
        ray's phase carried along.

        ``follow="ray"``: every ray is followed, its OPD changing by ``dopd`` and its point on the sphere by ``dpupil``
        -- the exact derivative of the sum ``psf()`` forms on the changed system with the sphere held fixed, the
        counterpart of ``rms_opd_gradient``.  ``follow="pupil"``: the wavefront change ``dfield`` at fixed pupil points,
        the sample positions held.  A ray is summed if ``psf()`` would keep it and its derivatives are finite for every
        parameter -- one set of rays for all parameters; the others are counted (``n_missed``, ``n_unfollowed``) and
        contribute nothing.  A ``WavelengthChange`` among the parameters is refused: it moves a ray between wavelengths.
        The weights are held, and so is every ray's path, as ``jacobian`` holds it."""
        self._need_wave("psf_gradient")
        import torch

        from . import engine

        unit = _positive(world_unit_um, "world_unit_um: how many micrometres one world unit is (1000 for mm)")
        nx, ny = _pixel_counts(pixels)
        step, uv0 = _pixel_grid(pixel_size, centre)
        values = self._wavelengths_for("psf_gradient", follow,
                                       "the PSF's derivative is taken for the other kinds of parameter")
        head = self._selected_rows()
        n_selected, n_groups, K = head.n_selected, head.n_groups, self.n_parameters
        dev = head.rows.device
        wave = self.wavefront
        f_number, step = _f_number_and_step(wave, values, unit, step, "psf_gradient")
        groups = np.ascontiguousarray(np.column_stack([wave.reference, wave.radius, wave.pivot, wave.pupil_radius]),
                                      dtype=np.float64)
        n_w = len(values)
        empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
        amplitude, damplitude = empty(n_groups, n_w, nx, ny, 2), empty(n_groups, K, n_w, nx, ny, 2)
        image, dimage = empty(n_groups, n_w, nx, ny), empty(n_groups, K, n_w, nx, ny)
        strehl, record = empty(n_groups, 1 + K), empty(n_groups, n_w, 5)
        lam = np.ascontiguousarray(values, dtype=np.float64)
        uv0 = np.ascontiguousarray(uv0)
        dphase = (self.dopd if follow == "ray" else self.dfield).contiguous()
        dpoint = self.dpupil.contiguous() if follow == "ray" else None
        engine.call("prt_frame_psf_gradient", *head, self.opd.contiguous(), self.pupil.contiguous(), groups, dphase, dpoint,
                    K, lam, n_w, unit, nx, ny, step[0], step[1], uv0, amplitude, damplitude, image, dimage, strehl, record,
                    device=dev, size=(n_selected, n_groups, K, n_w))
        return PSFGradient(engine.host_complex(amplitude), engine.host_complex(damplitude), engine.host(image),
                           engine.host(dimage), engine.host(strehl), engine.host(record), values, unit, (nx, ny), step,
                           (float(uv0[0]), float(uv0[1])), f_number, wave, self.parameters, follow)

    def rms_radius_at(self, parameters):
        """(groups, M): the RMS spot radius with the parameters changed by ``parameters`` (groups, M, K) under the linear
        ray model, every landing point moved by ``jacobian . p``: the quadratic
        ``mean_square + mean_square_gradient . p + p^T normal_matrix p`` of this object's sums, on the host -- about the
        moved centroid for ``reference="centroid"``, about the fixed point otherwise."""
        p = np.asarray(parameters, dtype=float)
        with np.errstate(invalid="ignore"):
            square = (self.mean_square[:, None] + np.einsum("gk,gmk->gm", self.mean_square_gradient, p)
                      + np.einsum("gmj,gjk,gmk->gm", p, self.normal_matrix, p))
            return np.sqrt(np.maximum(square, 0.0))

    def tolerance(self, trials, *, world_unit_um, compensators=(), follow="ray"):
        """Monte Carlo tolerancing from this one trace: the Strehl ratio and the RMS wavefront error of M perturbed
        systems, a ``ToleranceRun``.  Needs ``sensitivity(wavefront=)``.  Under the linear ray model every ray's OPD moves
        linearly in the parameters, ``OPD_r + sum_k dopd_rk p_k`` (``follow="ray"``, each ray followed; "pupil":
        ``dfield``, the pupil points held), while the merit stays fully nonlinear in the OPDs: the Strehl ratio of a
        trial is ``psf()``'s coherent sum on the moved OPDs, the sphere held fixed (``prt_frame_tolerance``;
        include/prt.h states the formulas) -- not ``strehl + dstrehl . p``.

        ``trials``: an (M, K) array of parameter changes, or a ``(Tolerances, M)`` pair to draw them; M <= 65535.
        ``compensators``: what is re-adjusted per trial and group so that the variance of the OPD over the pupil is
        least -- the index of a real parameter, or the pseudo-parameters "tilt" (the evaluation point moved by (du, dv)
        across the axis) and "focus" (by d delta along it), the extra columns ``-p1 / R``, ``-p2 / R`` and ``-p3 / R``
        with (p1, p2) = pupil * rho and p3 = -sign(u.a) sqrt(R^2 - p1^2 - p2^2) (``psf(focus=)``'s convention): the first-
        order change of d_r - R.  The minimiser comes from the covariance of the device's moments
        (``prt_frame_tolerance_moments``), solved on the host in longdouble (``solve_compensators``); the trial handed
        to the Strehl kernel carries it.  A ray is summed if ``psf()`` would keep it and every column is finite there;
        the others are counted (``n_missed``, ``n_unfollowed``).  A ``WavelengthChange`` among the parameters is refused.
        Second-order terms and rays whose path changes under a perturbation are out of scope."""
        self._need_wave("tolerance")
        import torch

        from . import engine

        unit = _positive(world_unit_um, "world_unit_um: how many micrometres one world unit is (1000 for mm)")
        K = self.n_parameters
        drawn = _drawn_trials(trials, K)
        if isinstance(compensators, (str, int, np.integer)):
            compensators = (compensators,)
        compensators = tuple(compensators)
        free, pseudo = [], []
        for c in compensators:
            if c in ("tilt", "focus"):
                pseudo.append(c)
            elif isinstance(c, (int, np.integer)) and not isinstance(c, bool) and 0 <= c < K:
                free.append(int(c))
            else:
                raise ValueError(f'compensators: indices of parameters (0..{K - 1}), "tilt" or "focus" (got {c!r})')
        if len(set(compensators)) != len(compensators):
            raise ValueError("compensators: each one once")
        values = self._wavelengths_for("tolerance", follow, "tolerances are taken for the other kinds of parameter")
        selected_rows = self._selected_rows()
        rows, n_selected, first, n_groups = (selected_rows.rows, selected_rows.n_selected, selected_rows.first,
                                             selected_rows.n_groups)
        dev = rows.device
        wave = self.wavefront
        # the columns: the K parameters, then the pseudo-parameters' (torch, on the device)
        columns = [(self.dopd if follow == "ray" else self.dfield)]
        if pseudo:
            first_t = torch.as_tensor(np.asarray(first, dtype=np.int64), device=dev)
            group = torch.repeat_interleave(torch.arange(n_groups, device=dev), first_t[1:] - first_t[:-1])
            radius = torch.as_tensor(np.asarray(wave.radius, dtype=np.float64), device=dev)[group]
            rho = torch.as_tensor(np.asarray(wave.pupil_radius, dtype=np.float64), device=dev)[group]
            p = self.pupil * rho[:, None]
            for c in pseudo:
                if c == "tilt":
                    columns.append((-p / radius[:, None]).T)
                else:
                    axis = torch.as_tensor(np.asarray(wave._made_of["axes"], dtype=np.float64).reshape(3, 3)[0], device=dev)
                    along = axis @ rows[_INDEX["x_tilt"]:_INDEX["z_tilt"] + 1][:, self._selected]
                    p3 = -torch.sign(along) * torch.sqrt(radius * radius - (p * p).sum(dim=1))
                    columns.append((-p3 / radius)[None, :])
        columns = torch.cat(columns, dim=0).contiguous()
        C = int(columns.shape[0])
        slots, at = [], K  # (the column of every compensator value, in the compensators' order)
        for c in compensators:
            if c == "tilt":
                slots += [at, at + 1]
                at += 2
            elif c == "focus":
                slots.append(at)
                at += 1
            else:
                slots.append(c)
        lam = np.ascontiguousarray(values, dtype=np.float64)
        n_w = len(lam)
        empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
        head = (*selected_rows, self.opd.contiguous(), columns, C, lam, n_w, unit)
        moments = empty(n_groups, 3 + (C + 2) * (C + 3) // 2)
        engine.call("prt_frame_tolerance_moments", *head, moments, device=dev, size=(n_selected, n_groups, C, n_w))
        moments = engine.host(moments)
        # per group: the covariance, the compensators of every trial (the nominal one last), the RMS of its OPD
        LD = np.longdouble
        M = len(drawn) + 1
        plain = np.zeros((M, C))
        plain[:-1, :K] = drawn
        q = np.full((n_groups, M, C), np.nan)
        rms_opd = np.full((n_groups, M), np.nan)
        for g in range(n_groups):
            covariance = moment_covariance(moments[g], C)
            if covariance is None:
                q[g] = plain
                continue
            qg, _ = solve_compensators(covariance, plain, slots)
            v = np.concatenate([np.ones((M, 1), dtype=LD), qg], axis=1)
            rms_opd[g] = np.sqrt(np.maximum(np.einsum("mi,ij,mj->m", v, covariance, v), 0)).astype(float)
            q[g] = qg.astype(float)
        handed = torch.as_tensor(np.ascontiguousarray(q), device=dev)
        strehl, amplitude, record = empty(n_groups, M), empty(n_groups, n_w, M, 2), empty(n_groups, n_w, 5)
        engine.call("prt_frame_tolerance", *head, handed, M, strehl, amplitude, record, device=dev,
                    size=(n_selected, n_groups, C, n_w, M))
        compensation = np.zeros((n_groups, M, len(slots)))
        for j, slot in enumerate(slots):  # (a real parameter: what was added to the drawn value)
            compensation[:, :, j] = q[:, :, slot] - (plain[:, slot] if slot < K else 0.0)
        rms_radius = np.full((n_groups, M), np.nan) if "focus" in pseudo else self.rms_radius_at(q[:, :, :K])
        return ToleranceRun(plain[:, :K], compensators, compensation, rms_opd, engine.host(strehl),
                            engine.host_complex(amplitude), rms_radius, engine.host(record), moments, values, unit,
                            self.parameters, follow)

    def mtf_tolerance(self, trials, frequencies, *, azimuths=(0.0, 90.0), focus=(0.0,), compensators=(),
                      reference="centroid", centre=None, axis=None, basis=None):
        """Monte Carlo tolerancing of the geometric MTF from this one trace: the OTF through focus of M perturbed
        systems, an ``MTFToleranceRun``.  Needs ``slopes`` (``sensitivity(slopes=True)``).  Under the linear ray model a
        ray lands at ``p + sum_k t_k dp_k`` with the slope ``s + sum_k t_k ds_k`` (``mtf_gradient()``'s staged
        quantities, about the same held centre, over the same kept rays), while the merit stays fully nonlinear in the
        moved points: the OTF of a trial is ``mtf()``'s sum on them (``prt_frame_mtf_tolerance``; include/prt.h states
        the formulas) -- not ``mtf + dmtf . t``.

        ``trials``: an (M, K) array of parameter changes, or a ``(Tolerances, M)`` pair to draw them; M <= 65535; the
        nominal all-zero trial is appended (``MTFToleranceRun.nominal``).  ``frequencies``, ``azimuths``, ``focus``,
        ``axis``, ``basis`` and ``centre`` as in ``mtf_gradient``.  ``compensators``: ``()`` or ``("focus",)``, the
        least-squares refocus of every trial from its own second moments, found on the device (a real parameter is
        compensated by the caller's own ``trials``).  ``reference="fixed"``: the kernel's numbers, about the held centre;
        ``"centroid"``: every trial about its own centroid, composed on the host as
        ``OTF exp(+2 pi i k.c_m(delta_f + delta_m))`` from the trial's moments -- what ``frame.mtf()`` of the perturbed
        system reports; |OTF| is the same under both.  A ``WavelengthChange`` may be among the parameters.  Second-order
        terms and rays whose path changes under a perturbation are out of scope."""
        self._need_slopes("mtf_tolerance")
        if reference not in ("fixed", "centroid"):
            raise ValueError('reference: "fixed" or "centroid"')
        if isinstance(compensators, str):
            compensators = (compensators,)
        try:
            compensators = tuple(compensators)
        except TypeError:
            compensators = (compensators,)
        if compensators not in ((), ("focus",)):
            raise ValueError(f'compensators: () or ("focus",) (got {compensators!r})')
        K = self.n_parameters
        drawn = _drawn_trials(trials, K)
        nu, theta, planes = _mtf_sampling(frequencies, azimuths, focus)
        axes = pupil_axes(axis, basis)
        head = self._selected_rows()
        centres = None if centre is None else _group_points(centre, head.n_groups, head.rows.device, "centre: None, a point")
        plain = np.concatenate([drawn, np.zeros((1, K))])
        trials = np.array(np.broadcast_to(plain[None], (head.n_groups,) + plain.shape), order="C")  # (the same for all)
        otf, moments, shift, record = _mtf_tolerance_run(head, self.jacobian, self.slopes, centres, axes, nu, theta, planes,
                                                         trials, bool(compensators))
        return MTFToleranceRun(plain, otf, moments, shift, record, nu, theta, planes, self.parameters, compensators,
                               reference)

    def energy_tolerance(self, trials, radii=None, *, fractions=(0.5, 0.8, 0.9), shape="circle", focus=(0.0,),
                         compensators=(), follow_centroid=True, centre=None, axis=None, basis=None):
        """Monte Carlo tolerancing of the geometric enclosed energy from this one trace: the energy within ``radii`` and
        the radius that holds each of ``fractions``, through focus, of M perturbed systems, an ``EnergyToleranceRun``.
        Needs ``slopes`` (``sensitivity(slopes=True)``).  The rays move under the linear ray model exactly as in
        ``mtf_tolerance`` (the same staged quantities, kept rays, held centre, moments and least-squares refocus, bit
        for bit), while the merit stays fully nonlinear in the moved points: every trial's energy is counted exactly
        with ``enclosed_energy``'s power-of-two integer weights, and its radius is a ray's own distance (the entry
        point of include/prt.h under the energy tolerancing states the formulas).

        ``trials``: an (M, K) array of parameter changes, or a ``(Tolerances, M)`` pair to draw them; M <= 65535; the
        nominal all-zero trial is appended (``EnergyToleranceRun.nominal``).  ``radii``: None or 1 to 256 values,
        finite, >= 0 and strictly ascending; ``fractions``: None or 1 to 16 values in (0, 1]; not both None; ``shape``
        and ``focus`` as in ``enclosed_energy``; ``compensators``: ``()`` or ``("focus",)`` as in ``mtf_tolerance``;
        ``centre``, ``axis`` and ``basis`` as in ``mtf_gradient``.  ``follow_centroid=True``: distances from the trial's
        own centroid in each plane, what ``enclosed_energy()`` of the perturbed system reports; ``False``: from the
        held centre -- the pixel or the fibre stays where it is while the spot walks off it, the case a decentre
        tolerance is about.  Second-order terms and rays whose path changes under a perturbation are out of scope."""
        self._need_slopes("energy_tolerance")
        from . import energy_tolerance

        if isinstance(compensators, str):
            compensators = (compensators,)
        try:
            compensators = tuple(compensators)
        except TypeError:
            compensators = (compensators,)
        if compensators not in ((), ("focus",)):
            raise ValueError(f'compensators: () or ("focus",) (got {compensators!r})')
        K = self.n_parameters
        drawn = _drawn_trials(trials, K)
        edges = np.zeros(0) if radii is None else _mtf_values(radii, "radii", 256, "finite, >= 0 and strictly ascending",
                                                              non_negative=True)
        if len(edges) > 1 and not np.all(np.diff(edges) > 0):
            raise ValueError("radii: 1 to 256 numbers, finite, >= 0 and strictly ascending")
        phi = np.zeros(0) if fractions is None else _mtf_values(fractions, "fractions", 16, "in (0, 1]")
        if np.any(phi <= 0) or np.any(phi > 1):
            raise ValueError("fractions: 1 to 16 numbers, in (0, 1]")
        if not len(edges) and not len(phi):
            raise ValueError("radii: give radii, fractions or both")
        if not isinstance(shape, str) or shape not in _ENERGY_SHAPES:
            raise ValueError(f"shape: one of {sorted(_ENERGY_SHAPES)} (got {shape!r})")
        planes = _mtf_values(focus, "focus", 256, "finite shifts along the axis")
        axes = pupil_axes(axis, basis)
        head = self._selected_rows()
        centres = None if centre is None else _group_points(centre, head.n_groups, head.rows.device, "centre: None, a point")
        plain = np.concatenate([drawn, np.zeros((1, K))])
        trials = np.array(np.broadcast_to(plain[None], (head.n_groups,) + plain.shape), order="C")  # (the same for all)
        count, energy, radius, moments, shift, record = energy_tolerance.device_run(
            head, self.jacobian, self.slopes, centres, axes, shape, follow_centroid, edges, phi, planes, trials,
            bool(compensators))
        return EnergyToleranceRun(plain, count, energy, radius, moments, shift, record, edges, phi, planes, self.parameters,
                                  shape, compensators, follow_centroid)

    def focus_gradient(self, axis=(1.0, 0.0, 0.0)):
        """(groups, K): the derivative of the least-squares best-focus shift along ``axis``, per parameter.  Past the
        surface a ray is a straight line; in the plane shifted by delta along the unit axis a it is at p + delta s, p the
        landing point and s = d / (d.a), both projected across a (the plane-shift convention of ``mtf(focus=)`` and
        ``enclosed_energy(focus=)``).  The weighted mean square radius about the centroid is least at
        delta = -cov(p, s) / var(s); this is d delta / d parameter, from ``jacobian`` (dp) and ``slopes`` (ds), over the
        selected rows that are finite in both, with the call's ``weights``.  For a ``WavelengthChange`` it is the
        chromatic focal shift per micrometre.  These are float64 torch reductions on the device: their bits are torch's
        and are NOT covered by the fixed-order contract of the sums.  NaN for a group without rows or with one slope."""
        import torch

        self._need_slopes("focus_gradient")
        rows, weights, first = (self._launch[k] for k in ("rows", "weights", "group_first"))
        try:
            a = np.asarray(axis, dtype=float).reshape(-1)
        except (TypeError, ValueError):
            a = np.zeros(0)
        if a.shape != (3,) or not np.all(np.isfinite(a)) or not np.linalg.norm(a) > 0:
            raise ValueError(f"axis: three finite numbers, not all zero (got {axis!r})")
        dev = self.jacobian.device
        a = torch.as_tensor(a / np.linalg.norm(a), dtype=torch.float64, device=dev)
        across = torch.eye(3, dtype=torch.float64, device=dev) - torch.outer(a, a)
        sel = self._selected
        x = rows[_INDEX["x1"]:_INDEX["z1"] + 1][:, sel]
        d = rows[_INDEX["x_tilt"]:_INDEX["z_tilt"] + 1][:, sel]
        d = d / torch.sqrt((d * d).sum(dim=0))
        w = rows[_INDEX[weights]][sel] if weights else torch.ones(len(sel), dtype=torch.float64, device=dev)
        da = a @ d
        p, s = across @ x, across @ (d / da)
        dp = torch.einsum("ab,kbn->kan", across, self.jacobian)
        ds = torch.einsum("ab,kbn->kan", across, self.slopes / da - d * (torch.einsum("b,kbn->kn", a, self.slopes) / (da * da))[:, None, :])
        keep = (torch.isfinite(w) & torch.isfinite(p).all(dim=0) & torch.isfinite(s).all(dim=0)
                & torch.isfinite(dp).all(dim=(0, 1)) & torch.isfinite(ds).all(dim=(0, 1)))
        out = np.full((len(first) - 1, self.n_parameters), np.nan)
        for g in range(len(first) - 1):
            at = slice(int(first[g]), int(first[g + 1]))
            k = keep[at]
            wg = w[at][k]
            total = wg.sum()
            if not int(k.sum()) or not float(total) > 0:
                continue
            pg, sg, dpg, dsg = p[:, at][:, k], s[:, at][:, k], dp[:, :, at][:, :, k], ds[:, :, at][:, :, k]
            pc = pg - (pg * wg).sum(dim=1, keepdim=True) / total
            sc = sg - (sg * wg).sum(dim=1, keepdim=True) / total
            cov = (wg * (pc * sc).sum(dim=0)).sum() / total
            var = (wg * (sc * sc).sum(dim=0)).sum() / total
            dcov = (wg * ((dpg * sc).sum(dim=1) + (dsg * pc).sum(dim=1))).sum(dim=1) / total
            dvar = 2 * (wg * (dsg * sc).sum(dim=1)).sum(dim=1) / total
            if float(var) > 0:
                out[g] = (-(dcov * var - cov * dvar) / (var * var)).cpu().numpy()
        return out

    def transfer(self, parameters_xy, parameters_uv, basis=None):
        """The 4x4 ray-transfer matrix about every selected ray: a device (n_selected, 4, 4) float64 tensor.
        ``parameters_xy``: the indices of two ``SourceMotion`` translations, ``parameters_uv``: of two rotations; the
        columns are per unit of those four parameters.  The rows are (x.e1, x.e2, d.e1, d.e2) of the landing point's and
        the direction's derivative in the transverse basis (e1, e2): ``basis``, or by default the unit vectors of the two
        translations (the launch's own transverse basis, right for a system that does not fold the axis).  For a
        translation by e and a rotation by 1 rad about a x e (a the axis) these are the blocks A, B / C, D of first-order
        optics, about the real ray, not the axis.  Index arithmetic on ``jacobian`` and ``slopes``."""
        import torch

        self._need_slopes("transfer")
        picked = []
        for name, pair in (("parameters_xy", parameters_xy), ("parameters_uv", parameters_uv)):
            pair = list(pair)
            if len(pair) != 2 or not all(isinstance(k, (int, np.integer)) and 0 <= k < self.n_parameters
                                         and isinstance(self.parameters[k], SourceMotion) for k in pair):
                raise ValueError(f"transfer: {name} is the indices of two SourceMotions among the parameters")
            picked += [int(k) for k in pair]
        if basis is None:
            basis = [self.parameters[k].translate for k in picked[:2]]
        e = np.asarray(basis, dtype=float)
        if e.shape != (2, 3) or not np.all(np.isfinite(e)) or not np.all(np.linalg.norm(e, axis=1) > 0):
            raise ValueError("transfer: basis is two vectors that are not zero (by default the translations of parameters_xy)")
        e = torch.as_tensor(e / np.linalg.norm(e, axis=1, keepdims=True), dtype=torch.float64, device=self.jacobian.device)
        top = torch.einsum("ac,kcn->nak", e, self.jacobian[picked])
        bottom = torch.einsum("ac,kcn->nak", e, self.slopes[picked])
        return torch.cat([top, bottom], dim=1)

    def effective_focal_length(self, parameter, axis=(1.0, 0.0, 0.0)):
        """(groups,): the effective focal length from a collimated source along ``axis`` whose field angle is parameter
        ``parameter``, a ``SourceMotion`` rotation: d(centroid)/d(field angle) along the direction the beam tilts in,
        ``centroid_gradient[:, k].t / |rotate x a|`` with t the unit vector of rotate x a -- the weighted mean of the
        block B of ``transfer`` over the group.  On a detector in the focal plane of a lens without a fold this is f
        (the image of a beam at the angle theta is at f tan(theta)); its change over the field is the distortion."""
        k = parameter
        if not (isinstance(k, (int, np.integer)) and 0 <= k < self.n_parameters and isinstance(self.parameters[k], SourceMotion)):
            raise ValueError("effective_focal_length: parameter is the index of a SourceMotion among the parameters")
        a = np.asarray(axis, dtype=float).reshape(-1)
        if a.shape != (3,) or not np.all(np.isfinite(a)) or not np.linalg.norm(a) > 0:
            raise ValueError(f"axis: three finite numbers, not all zero (got {axis!r})")
        tilt = np.cross(self.parameters[k].rotate, a / np.linalg.norm(a))
        rate = np.linalg.norm(tilt)
        if not rate > 0:
            raise ValueError("effective_focal_length: the parameter does not tilt a beam along axis (rotate x axis is zero)")
        return self.centroid_gradient[:, k] @ (tilt / rate) / rate

    def rows(self):
        """The frame rows of the selection, in the order of ``jacobian``'s last axis: a device int64 tensor."""
        return self._selected

    def step(self, damping=0.0, merit="spot"):
        """Per group the change of the parameters that minimises the mean square radius to first order (Gauss-Newton
        on the landing points): the solution of (N + damping diag(N)) dp = rhs through ``solve_normal_equations``
        (the minimum-norm one where the rays cannot tell the parameters apart).  (groups, K); NaN without rows.
        ``merit="wavefront"`` (with ``sensitivity(wavefront=)``): Gauss-Newton on the piston-removed OPD with ``dfield``
        as the Jacobian, which minimises the wavefront variance to first order."""
        if not (np.isfinite(damping) and damping >= 0):
            raise ValueError("damping: a number >= 0")
        if merit not in ("spot", "wavefront"):
            raise ValueError('merit: "spot" or "wavefront"')
        K = self.n_parameters
        if merit == "wavefront":
            self._need_wave('step(merit="wavefront")')
            return self._solve(self.wavefront_normal_matrix, self.wavefront_rhs, self._wave_weight, damping)
        return self._solve(self.normal_matrix, self.rhs, self.weight, damping)

    def _solve(self, normal_matrix, rhs, weight, damping):
        K = self.n_parameters
        upper = np.triu_indices(K)
        packed = np.zeros((len(self.sums), len(upper[0]) + K + 3))
        for g in range(len(packed)):
            if not np.all(np.isfinite(normal_matrix[g])) or not np.all(np.isfinite(rhs[g])):
                continue
            a = normal_matrix[g] + damping * np.diag(np.diag(normal_matrix[g]))
            packed[g, :len(upper[0])] = a[upper]
            packed[g, len(upper[0]):len(upper[0]) + K] = rhs[g]
            packed[g, -3] = weight[g]
        return solve_normal_equations(packed, K)[0]

    def to_pandas(self):
        """One line per selected row: ``row``, then ``dx_k``, ``dy_k``, ``dz_k`` per parameter k."""
        from . import engine

        data = {"row": engine.to_host(self._selected).copy()}
        jac = engine.to_host(self.jacobian)
        for k in range(self.n_parameters):
            for c, name in enumerate("xyz"):
                data[f"d{name}_{k}"] = jac[k, c].copy()
        return pd.DataFrame(data)


# --- what DeviceFrame.sensitivity() is made of ---------------------------------------------------------------------------
# The arguments of the four entry points, by name and in the order of include/prt.h: each form is what its size function
# takes after (n_ids, n_surfaces, K, n_groups, max_group_rows), its entry point, and the pieces of its call, which
# engine.call ends with the workspace and the stream.
_SENS_COMMON = ("device", "rows", "ld", "counts", "n_generations", "id0", "n_ids", "prims", "n_prims", "twists",
              "parameter_ids", "parameter_first")
_SENS_DESIGN = ("linear", "index_rates", "index_ids", "index_first")
_SENS_SELECTION = ("K", "row_slot", "selected", "n_selected", "group_first", "n_groups", "weight_column", "pivots")
_SENS_WAVE_IN = ("opl", "groups", "axes", "n_terms")
_SENS_LAUNCH_IN = ("ranges", "flags", "colour_rates", "materials", "n_materials")
_SENS_WAVE_OUT = ("dfield", "dopd", "dpupil", "opd", "pupil", "opd_sums")
_SENS_FORMS = {
    "rigid": ((), "prt_frame_sensitivity", _SENS_COMMON + _SENS_SELECTION + ("jacobian", "sums", "record")),
    "design": ((), "prt_frame_design_sensitivity",
               _SENS_COMMON + _SENS_DESIGN + _SENS_SELECTION + ("jacobian", "sums", "record")),
    "wavefront": (("n_terms",), "prt_frame_opd_sensitivity",
                  _SENS_COMMON + _SENS_DESIGN + _SENS_SELECTION + _SENS_WAVE_IN + ("jacobian", "sums") + _SENS_WAVE_OUT
                  + ("record",)),
    "launch": (("n_terms",), "prt_frame_launch_sensitivity",
               _SENS_COMMON + _SENS_DESIGN + _SENS_SELECTION + _SENS_WAVE_IN + _SENS_LAUNCH_IN
               + ("jacobian", "sums", "slopes") + _SENS_WAVE_OUT + ("record",)),
}


# --- how a pass reaches the library: engine.call, after these leading arguments -------------------
def _row_head(rows):
    """``(device index, rows, ld, n_rows)`` of a (15, n) block, contiguous along the row axis: what every pass over rows
    begins with.  A contiguous block has the stride n (1 when it is empty), a view of a larger one the larger stride."""
    n_rows = rows.shape[1]
    return rows.device.index or 0, rows, max(rows.stride(0), n_rows, 1), n_rows


def _row_filter(surface, generation, rays_per_source, n_groups):
    """``(surface, generation, rays_per_source, n_groups)`` as the passes read the selection: NaN for a surface or a
    generation that does not filter, 0 rays a source for one group."""
    surface, generation = [float("nan") if value is None else float(value) for value in (surface, generation)]
    return surface, generation, float(rays_per_source or 0), n_groups


def _weight_column(weights):
    """The column the weights are read from, -1 for ones."""
    return -1 if weights is None else _INDEX[weights]


# (what psf() tells the results of its three sums of the grid, and the leading arguments of Sensitivity._selected_rows)
_HuygensGrid = namedtuple("_HuygensGrid", "wavelengths unit pixels step centre f_number wave")
_SelectedRows = namedtuple("_SelectedRows", "device rows ld n_rows selected n_selected first n_groups weight_column")


def _sens_parameters(parameters, rays_per_source, slopes):
    """``(motions, form)``: the parameters as a list, every ``SourceMotion``'s rays resolved, and what they ask of the
    call -- ``design``: not Motions alone; ``launch``: a SourceMotion or a WavelengthChange; ``colour``: a
    WavelengthChange; ``launch_form``: the entry point that also writes the slopes."""
    kinds = (Motion, Deformation, IndexChange, SourceMotion, WavelengthChange)
    motions = [parameters] if isinstance(parameters, kinds) else list(parameters)
    if not motions or not all(isinstance(m, kinds) for m in motions):
        raise ValueError("sensitivity: parameters is a Motion, a Deformation, an IndexChange, a SourceMotion or a "
                         "WavelengthChange, or a list of them")
    form = dict(design=not all(isinstance(m, Motion) for m in motions),
                launch=any(isinstance(m, (SourceMotion, WavelengthChange)) for m in motions),
                colour=any(isinstance(m, WavelengthChange) for m in motions))
    form["launch_form"] = form["launch"] or bool(slopes)
    if len(motions) > 16:
        raise ValueError(f"sensitivity: at most 16 parameters a call (got {len(motions)})")
    if form["launch"]:
        motions = [m.resolved(rays_per_source) if isinstance(m, SourceMotion) else m for m in motions]
    return motions, form


def _sens_primitives(system, motions, colour):
    """``(snapshot, prims)``: the snapshot of ``system`` (the components, or their ``SceneSnapshot``) and its primitives
    sorted by surface id.  The ids are distinct, every surface a parameter names is among them, and with a
    ``WavelengthChange`` (``colour``) no glass is a table glass: ``ValueError`` otherwise."""
    from . import materials as matl
    from .scene import PRIM_DTYPE, SceneSnapshot

    snapshot = system if hasattr(system, "prims") else SceneSnapshot(system)
    prims = np.sort(np.asarray(snapshot.prims, dtype=PRIM_DTYPE), order="surface_id")
    if len(prims) == 0:
        raise ValueError("sensitivity: system has no surfaces")
    if len(np.unique(prims["surface_id"])) != len(prims):
        raise ValueError("sensitivity: a surface id repeats in system")
    known = set(int(v) for v in prims["surface_id"])
    for k, motion in enumerate(motions):
        missing = sorted(set(motion.surface_ids) - known)
        if missing:
            raise ValueError(f"sensitivity: parameter {k} moves surfaces that are not in system: {missing}")
    if colour and any(int(kind) == matl.TABLE for kind in np.asarray(snapshot.materials)["kind"][prims["material"]]):
        raise ValueError("sensitivity: a WavelengthChange needs the dispersion of every glass in system, and a table "
                         "glass's index_at is host code without a derivative")
    return snapshot, prims


def _sens_made_of(wavefront, mine):
    """What ``wavefront`` was made of (``Wavefront._made_of``), held to this call's frame, surface, generation, groups
    and weights (``mine``): ``ValueError`` for a Wavefront of anything else."""
    made = getattr(wavefront, "_made_of", None)
    if made is None:
        raise ValueError("sensitivity: wavefront was not made by this frame's wavefront()")
    for name, value in mine.items():
        if (made[name] is not value) if name == "frame" else (made[name] != value):
            raise ValueError(f"sensitivity: wavefront is of another {name} ({made[name]!r}, this call: {value!r}): "
                             "it must be this frame's, at the same surface, generation, groups and weights")
    return made


def _sens_selection(rows, surface_id, generation, rays_per_source, n_groups, id0, n_ids, n_generations):
    """``(selected, row_slot, group_first)``: the rows that end on the surface (of ``generation``, where given) in the
    order (group, generation, id) -- what makes the sums independent of the rows' order --, per row its slot in that
    selection or -1, and on the host the first slot of every group and the end (a read that waits for the stream)."""
    import torch

    dev = rows.device
    mask = rows[_INDEX["surface"]] == surface_id
    if generation is not None:
        mask = mask & (rows[_INDEX["generation"]] == float(generation))
    ids = rows[_INDEX["id"]]
    group = torch.zeros_like(ids, dtype=torch.int64)
    if rays_per_source:
        group = torch.floor(ids / float(rays_per_source)).to(torch.int64)
    mask = mask & (group >= 0) & (group < n_groups)
    picked = torch.nonzero(mask).reshape(-1)
    key = ((group[picked] * max(n_generations, 1) + rows[_INDEX["generation"]][picked].to(torch.int64)) * n_ids
           + (ids[picked] - id0).to(torch.int64))
    selected = picked[torch.argsort(key)].contiguous()
    row_slot = torch.full((max(rows.shape[1], 1),), -1, dtype=torch.int64, device=dev)
    row_slot[selected] = torch.arange(selected.shape[0], dtype=torch.int64, device=dev)
    group_first = torch.searchsorted(group[selected].contiguous(), torch.arange(n_groups + 1, dtype=torch.int64, device=dev))
    return selected, row_slot, np.ascontiguousarray(group_first.cpu().numpy(), dtype=np.int64)


def _sens_pivots(rows, reference, selected, group_first, n_groups):
    """``(pivots, centred)``: per group the point its sums are taken about, (n_groups, 3) on the host.  "centroid"
    (``centred``): a point of the group, its first row's (a read that waits for the stream) -- the centroid follows from
    the sums; else the reference itself, a point or one a group."""
    import torch

    centred = isinstance(reference, str)
    if centred:
        pivots = np.zeros((n_groups, 3))
        some = np.flatnonzero(np.diff(group_first) > 0)
        if len(some):
            first_rows = selected[torch.as_tensor(group_first[some], device=rows.device)]
            pivots[some] = rows[_INDEX["x1"]:_INDEX["z1"] + 1][:, first_rows].T.cpu().numpy()
        pivots[~np.isfinite(pivots)] = 0.0
    else:
        pivots = np.asarray(reference.cpu() if hasattr(reference, "cpu") else reference, dtype=float)
        if pivots.shape == (3,):
            pivots = np.broadcast_to(pivots, (n_groups, 3))
        if pivots.shape != (n_groups, 3) or not np.all(np.isfinite(pivots)):
            raise ValueError(f"reference: \"centroid\", a finite point or an ({n_groups}, 3) array")
    return np.ascontiguousarray(pivots, dtype=np.float64), centred


def _packed_ids(id_lists):
    """``(ids, first)``: one list of surface ids a parameter as the library reads them -- the ids end to end (int64; a
    single 0 where there are none) and, int32, where each parameter's begin and the last one's end."""
    first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(v) for v in id_lists])]), dtype=np.int32)
    return np.ascontiguousarray([v for ids in id_lists for v in ids] or [0], dtype=np.int64), first


def _sens_host_arrays(motions, form, materials):
    """The parameters packed for the entry point of ``form`` ("rigid", "design", "wavefront", "launch"), by the names of
    ``_SENS_FORMS``: the twists and the surfaces each parameter moves; but for the rigid form S, the index rates and the
    surfaces whose index each changes; for the launch form the rays each parameter names, what it does to them and the
    glasses.  A parameter that has no such part has zeros and an empty list there."""
    def rows_of(kind, value, zero):
        return [value(m) if isinstance(m, kind) else zero for m in motions]

    host = dict(twists=np.ascontiguousarray(rows_of((Motion, Deformation, SourceMotion), lambda m: m.twist, np.zeros(9)),
                                            dtype=np.float64))
    host["parameter_ids"], host["parameter_first"] = _packed_ids(
        rows_of((Motion, Deformation, SourceMotion), lambda m: sorted(m.surface_ids), []))
    if form != "rigid":
        host["linear"] = np.ascontiguousarray(rows_of(Deformation, lambda m: m.linear.reshape(-1), np.zeros(9)),
                                              dtype=np.float64)
        host["index_rates"] = np.ascontiguousarray(rows_of(IndexChange, lambda m: m.rate, 0.0), dtype=np.float64)
        host["index_ids"], host["index_first"] = _packed_ids(rows_of(IndexChange, lambda m: sorted(m.surface_ids), []))
    if form == "launch":
        host["ranges"] = np.ascontiguousarray(rows_of((SourceMotion, WavelengthChange), lambda m: m.id_range, (0.0, 0.0)),
                                              dtype=np.float64)
        host["flags"] = np.ascontiguousarray([1 if isinstance(m, SourceMotion) else 2 if isinstance(m, WavelengthChange)
                                              else 0 for m in motions], dtype=np.int32)
        host["colour_rates"] = np.ascontiguousarray(rows_of(WavelengthChange, lambda m: m.rate, 0.0), dtype=np.float64)
        host["materials"] = np.ascontiguousarray(materials)
        host["n_materials"] = len(host["materials"])
    return host


def _coating_stacks(coatings, ids_lossless):
    """``coatings`` of ``fresnel()`` as (the distinct Coatings, {surface id: its number among them})."""
    from .materials import Coating

    if not hasattr(coatings, "items"):
        raise ValueError("fresnel: coatings is a mapping from a surface to a Coating")
    stacks, surface_coating = [], {}
    for key, coating in coatings.items():
        if not isinstance(coating, Coating):
            raise ValueError(f"fresnel: coatings maps a surface to a Coating (got {coating!r})")
        known = [k for k, other in enumerate(stacks) if other is coating]
        if not known:
            stacks.append(coating)
        for sid in sorted(_lossless_ids(key)):
            if sid in surface_coating:
                raise ValueError(f"fresnel: surface {sid} is given two coatings")
            surface_coating[sid] = known[0] if known else len(stacks) - 1
    both = sorted(set(surface_coating) & set(ids_lossless))
    if both:
        raise ValueError(f"fresnel: surfaces {both} are both lossless and coated")
    if len(surface_coating) > 64:
        raise ValueError(f"fresnel: at most 64 coated surfaces (got {len(surface_coating)})")
    if len(stacks) > 16:
        raise ValueError(f"fresnel: at most 16 coatings (got {len(stacks)})")
    return stacks, surface_coating


def _coating_tables(stacks, surface_coating, rows):
    """The table arguments of ``prt_frame_fresnel_coated``, in its order: the materials on the distinct wavelengths of
    the frame (as DeviceScene.ensure_tables does for table glasses)."""
    import torch

    from . import engine

    wavelengths = np.zeros(0)
    if stacks and rows is not None:
        wavelengths = engine.to_host(torch.unique(rows[_INDEX["wavelength"]])).astype(np.float64)
        wavelengths = np.ascontiguousarray(wavelengths[np.isfinite(wavelengths) & (wavelengths > 0)])
        if len(wavelengths) > 256:
            raise ValueError(f"fresnel: at most 256 distinct wavelengths with coatings (got {len(wavelengths)})")
    table = np.ones((max(len(stacks), 1), 18, max(len(wavelengths), 1)), dtype=np.complex128)
    thickness = np.zeros((max(len(stacks), 1), 16))
    for k, coating in enumerate(stacks):
        if len(wavelengths):
            table[k] = coating.table(wavelengths)
        thickness[k, :len(coating.layers)] = [d for _, d in coating.layers]
    table = np.ascontiguousarray(table).view(np.float64)
    layer_counts = np.array([len(c.layers) for c in stacks] or [0], dtype=np.int32)
    has_substrate = np.array([c.substrate is not None for c in stacks] or [0], dtype=np.int32)
    coated_ids = np.array(sorted(surface_coating) or [0], dtype=np.int64)
    coating_of = np.array([surface_coating[sid] for sid in sorted(surface_coating)] or [0], dtype=np.int32)
    return (coated_ids, coating_of, len(surface_coating), len(stacks), layer_counts, has_substrate, thickness,
            wavelengths if len(wavelengths) else None, len(wavelengths), table)


def _lossless_ids(items):
    """Surface ids of ``lossless``: ids, objects with ``get_id()``, components with ``surface_ids``, or several of them."""
    if items is None:
        return set()
    if isinstance(items, (str, bytes)) or hasattr(items, "get_id") or hasattr(items, "surface_ids") or not hasattr(items, "__iter__"):
        items = (items,)
    out = set()
    for item in items:
        if hasattr(item, "surface_ids"):
            out.update(int(sid) for sid, _ in item.surface_ids)
        else:
            out.add(int(_surface_id(item)))
    return out


def _surface_id(item):
    return item.get_id() if hasattr(item, "get_id") else item


def _surface_ids(items):
    if items is None:
        return set()
    if isinstance(items, (str, bytes)) or hasattr(items, "get_id") or not hasattr(items, "__iter__"):
        items = (items,)
    return {_surface_id(item) for item in items}


def diffraction_mtf(frequencies, wavelength_um, f_number, world_unit_um):
    """The diffraction-limited MTF of a circular pupil without aberrations: (2 / pi) (phi - cos phi sin phi) with
    phi = arccos(nu lambda F), and 0 past the cutoff nu = 1 / (lambda F).  frequencies in cycles per world unit,
    wavelength in micrometres, world_unit_um: how many micrometres one world unit is (1000 for mm)."""
    unit = _positive(world_unit_um, "world_unit_um: how many micrometres one world unit is (1000 for mm)")
    lam = _positive(wavelength_um, "wavelength_um: finite and > 0") / unit
    f = _positive(f_number, "f_number: finite and > 0")
    nu = np.asarray(frequencies, dtype=float)
    if not np.all(np.isfinite(nu) & (nu >= 0)):
        raise ValueError("frequencies: finite and >= 0")
    x = np.minimum(nu * lam * f, 1.0)
    phi = np.arccos(x)
    return (2 / np.pi) * (phi - np.cos(phi) * np.sin(phi))


def _mtf_values(values, name, cap, rule, non_negative=False):
    """A 1-D float64 array of 1..cap finite values (>= 0 when non_negative)."""
    try:
        array = np.ascontiguousarray(np.atleast_1d(np.asarray(values, dtype=np.float64)))
    except (TypeError, ValueError):
        raise ValueError(f"{name}: 1 to {cap} numbers, {rule} (got {values!r})") from None
    if array.ndim != 1 or not 1 <= len(array) <= cap:
        raise ValueError(f"{name}: 1 to {cap} numbers, {rule} (got {array.size})")
    if not np.all(np.isfinite(array)) or (non_negative and np.any(array < 0)):
        raise ValueError(f"{name}: 1 to {cap} numbers, {rule}")
    return array


def _mtf_sampling(frequencies, azimuths, focus):
    """The frequencies, azimuths and focus shifts of ``mtf()`` and ``mtf_gradient()`` as arrays."""
    return (_mtf_values(frequencies, "frequencies", 4096, "finite and >= 0", non_negative=True),
            _mtf_values(azimuths, "azimuths", 16, "finite, in degrees"),
            _mtf_values(focus, "focus", 256, "finite shifts along the axis"))


def _check_weights(weights):
    if weights is not None and weights not in _INDEX:
        raise ValueError(f"weights: None or a column name (got {weights!r})")


def _check_reference_name(reference):
    if isinstance(reference, str) and reference != "centroid":
        raise ValueError('reference: "centroid", a point or an (n_groups, 3) array')


def _group_count(rays_per_source, n_groups, top):
    """The number of groups ``id // rays_per_source`` of a pass: ``n_groups`` where it is given, else counted from the
    largest ray id ``top()``, read only then; 1 without ``rays_per_source``."""
    if not rays_per_source:
        return 1
    return max(1, int(top() // rays_per_source) + 1) if n_groups is None else n_groups


def _group_points(value, n_groups, device, rule):
    """A point, or one per group, as an (n_groups, 3) float64 tensor on ``device``.  ``rule``: the argument's name and
    what else it takes, the head of the message."""
    import torch

    points = torch.as_tensor(np.asarray(value.cpu() if hasattr(value, "cpu") else value, dtype=float))
    if points.shape == (3,):
        points = points.expand(n_groups, 3)
    if tuple(points.shape) != (n_groups, 3):
        raise ValueError(f"{rule} or an ({n_groups}, 3) array (got shape {tuple(points.shape)})")
    return points.to(device, torch.float64).contiguous()


def _positions(sampled, wanted, name):
    """Indices of the wanted values among the sampled ones."""
    out = []
    for value in np.atleast_1d(np.asarray(wanted, dtype=float)):
        hits = np.flatnonzero(np.isclose(sampled, value, rtol=1e-12, atol=0))
        if not len(hits):
            raise ValueError(f"{name}: {value} is not one of the sampled values {list(sampled)}")
        out.append(int(hits[0]))
    return out


def _positive(value, message):
    try:
        number = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{message} (got {value!r})") from None
    if not (np.isfinite(number) and number > 0):
        raise ValueError(f"{message} (got {value!r})")
    return number


def _pixel_counts(pixels):
    """pixels: an int or (nx, ny), each 1..1024."""
    pair = (pixels, pixels) if np.ndim(pixels) == 0 else tuple(pixels)
    if len(pair) != 2 or not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 1 <= k <= 1024
                                 for k in pair):
        raise ValueError(f"pixels: an int or (nx, ny), each 1..1024 (got {pixels!r})")
    return int(pair[0]), int(pair[1])


def _pixel_grid(pixel_size, centre):
    """pixel_size: a number, (du, dv) or None; centre: (u0, v0).  Returns the step (None: the default) and the centre."""
    step = None
    if pixel_size is not None:
        pair = np.asarray(pixel_size, dtype=float).reshape(-1)
        pair = np.repeat(pair, 2) if pair.size == 1 else pair
        if pair.shape != (2,) or not np.all(np.isfinite(pair)) or not np.all(pair > 0):
            raise ValueError(f"pixel_size: a positive number or (du, dv), or None (got {pixel_size!r})")
        step = (float(pair[0]), float(pair[1]))
    uv0 = np.asarray(centre, dtype=float)
    if uv0.shape != (2,) or not np.all(np.isfinite(uv0)):
        raise ValueError(f"centre: (u0, v0), finite (got {centre!r})")
    return step, uv0


def _distinct_wavelengths(values, name):
    """The distinct wavelengths of the selected rows as the Huygens passes take them: finite, > 0, at most 16."""
    if not np.all(np.isfinite(values) & (values > 0)):
        raise ValueError(f"{name}: a selected row's wavelength is not finite and > 0")
    if len(values) > 16:
        raise ValueError(f"{name}: at most 16 distinct wavelengths (the selected rows hold {len(values)})")
    return values


def _mtf_tolerance_run(head, jacobian, slopes, centres, axes, frequencies, azimuths, planes, trials, compensate_focus):
    """``prt_frame_mtf_tolerance`` on the selected rows ``head`` and host ``trials`` (groups, M, K), which may differ by
    group.  Returns host arrays: otf (groups, M, F, A, N) complex, moments (groups, M, 8), focus_shift (groups, M), record
    (groups, 7)."""
    import torch

    from . import engine

    dev, n_groups = head.rows.device, head.n_groups
    trials = np.ascontiguousarray(trials, dtype=np.float64)
    M, K = trials.shape[1:]
    assert trials.shape[0] == n_groups and K == jacobian.shape[0], (trials.shape, n_groups, jacobian.shape)
    shape = (len(planes), len(azimuths), len(frequencies))
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    otf, moments, shift, record = empty(n_groups, M, *shape, 2), empty(n_groups, M, 8), empty(n_groups, M), empty(n_groups, 7)
    engine.call("prt_frame_mtf_tolerance", *head, jacobian.contiguous(), slopes.contiguous(), K, centres, axes, frequencies,
                len(frequencies), azimuths, len(azimuths), planes, len(planes), torch.as_tensor(trials, device=dev), M,
                int(bool(compensate_focus)), otf, moments, shift, record, device=dev,
                size=(head.n_selected, n_groups, K, len(frequencies), len(azimuths), len(planes), M))
    return engine.host_complex(otf), engine.host(moments), engine.host(shift), engine.host(record)


def _drawn_trials(trials, K):
    """``trials`` of ``tolerance`` and ``mtf_tolerance`` as a finite (M, K) float64 array, 1 <= M <= 65535: the array
    itself, or M draws of a ``(Tolerances, M)`` pair."""
    if isinstance(trials, tuple) and len(trials) == 2 and isinstance(trials[0], Tolerances):
        if len(trials[0].widths) != K:
            raise ValueError(f"trials: the Tolerances have {len(trials[0].widths)} widths for {K} parameters")
        trials = trials[0].sample(trials[1])
    try:
        drawn = np.array(trials, dtype=np.float64)
    except (TypeError, ValueError):
        drawn = np.zeros(0)
    if drawn.ndim != 2 or drawn.shape[1] != K or not 1 <= drawn.shape[0] <= 65535 or not np.all(np.isfinite(drawn)):
        raise ValueError(f"trials: a finite (M, {K}) array, 1 <= M <= 65535, or a (Tolerances, M) pair")
    return drawn


def _f_number_and_step(wave, wavelengths, unit, step, name):
    """F = R / (2 rho_max) per group (NaN without rays); the step: the caller's, or lambda_min * F_min / 4 both ways."""
    n_rays, radius, rho = (np.asarray(v) for v in (wave.n_rays, wave.radius, wave.pupil_radius))
    with np.errstate(invalid="ignore", divide="ignore"):
        f_number = np.where(n_rays > 0, radius / (2.0 * rho), np.nan)
    if step is None:
        finite = f_number[np.isfinite(f_number) & (f_number > 0)]
        if not len(finite):
            raise ValueError(f"{name}: no group has rays that meet the reference sphere; give pixel_size")
        step = (float(wavelengths.min()) / unit * float(finite.min()) / 4.0,) * 2
    return f_number, step


RANK_RCOND = 1e-10  # singular values of Z^T W Z below this share of the largest are dropped (of Z: below 1e-5)


def solve_normal_equations(normal, terms):
    """Per group the least-squares Zernike coefficients from the device's sums (``numpy.linalg.lstsq`` on the J x J
    system: the minimum-norm solution where the pupil fill leaves the terms dependent) and the system's effective
    rank (``RANK_RCOND``: the normal equations square the design matrix's condition, so lstsq's default cut-off
    would count rounding noise as rank)."""
    normal = np.atleast_2d(np.asarray(normal, dtype=float))
    upper = np.triu_indices(terms)
    tri = len(upper[0])
    coefficients = np.full((normal.shape[0], terms), np.nan)
    rank = np.zeros(normal.shape[0], dtype=np.int64)
    for g, sums in enumerate(normal):
        if not sums[-3] > 0:
            continue
        a = np.zeros((terms, terms))
        a[upper] = sums[:tri]
        a = a + np.triu(a, 1).T
        coefficients[g], _, rank[g], _ = np.linalg.lstsq(a, sums[tri:tri + terms], rcond=RANK_RCOND)
    return coefficients, rank


def noll_index(j):
    """Noll's (1976) single index j = 1, 2, ... -> (n, m): m > 0 for cos(m theta) (even j), m < 0 for sin (odd j)."""
    if j < 1:
        raise ValueError("Noll indices start at 1")
    n, k = 0, j - 1
    while k > n:
        n += 1
        k -= n
    m = n % 2 + 2 * ((k + (n + 1) % 2) // 2)
    return n, (-m if j % 2 else m)


def zernike_basis(terms, rho, theta):
    """Z_1 .. Z_terms (Noll's order and RMS normalisation) at (rho, theta): an array of shape (terms,) + rho's
    shape.  The host statement of what ``k_frame_zernike`` evaluates (there by recurrence)."""
    from math import factorial

    rho, theta = np.asarray(rho, dtype=float), np.asarray(theta, dtype=float)
    out = []
    for j in range(1, terms + 1):
        n, m = noll_index(j)
        am = abs(m)
        radial = sum((-1) ** k * factorial(n - k) / (factorial(k) * factorial((n + am) // 2 - k)
                                                     * factorial((n - am) // 2 - k)) * rho ** (n - 2 * k)
                     for k in range((n - am) // 2 + 1))
        norm = np.sqrt(n + 1.0) if m == 0 else np.sqrt(2.0 * (n + 1))
        angular = 1.0 if m == 0 else (np.cos(am * theta) if m > 0 else np.sin(am * theta))
        out.append(norm * radial * angular)
    return np.array(out)


def pupil_axes(axis=None, basis=None):
    """The 9 doubles (a, e1, e2) the pupil projection uses: a unit axis and an orthonormal basis of the plane
    perpendicular to it.  Default: a = x, e1 = y, e2 = z.  An axis without a basis gets e1 from y (z when the axis
    is along y) made perpendicular to it, and e2 = a x e1."""
    a = np.array((1.0, 0.0, 0.0) if axis is None else axis, dtype=float)
    if a.shape != (3,) or not np.all(np.isfinite(a)) or not np.linalg.norm(a) > 0:
        raise ValueError("axis: a finite, non-zero 3-vector")
    a = a / np.linalg.norm(a)
    if basis is None:
        if axis is None:
            e1, e2 = np.array((0.0, 1.0, 0.0)), np.array((0.0, 0.0, 1.0))
        else:
            seed = np.array((0.0, 1.0, 0.0)) if abs(a[1]) < 0.9 else np.array((0.0, 0.0, 1.0))
            e1 = seed - np.dot(seed, a) * a
            e1 /= np.linalg.norm(e1)
            e2 = np.cross(a, e1)
    else:
        e1, e2 = (np.array(e, dtype=float) for e in basis)
        if e1.shape != (3,) or e2.shape != (3,):
            raise ValueError("basis: two 3-vectors (e1, e2)")
        frame = np.stack([a, e1, e2])
        if not np.allclose(frame @ frame.T, np.eye(3), atol=1e-9):
            raise ValueError("basis: e1, e2 must be unit vectors perpendicular to each other and to the axis")
    return np.ascontiguousarray(np.concatenate([a, e1, e2]), dtype=np.float64)


def histogram_edges(bins, range, dims, finite_range):
    """The bin edges numpy's np.histogram (dims 1) / np.histogram2d (dims 2) would use, with numpy's own errors, and per
    axis whether they are evenly spaced (bins given as a count).  finite_range(axis) -> (lo, hi): the range of an axis
    whose bins are a count and whose range is None (numpy would take the data's min and max)."""
    if isinstance(bins, str):
        raise ValueError(f"string bin estimators ({bins!r}) are not supported: give a number of bins or the edges")
    if dims == 1:
        uniform = np.ndim(bins) == 0
        if uniform and range is None:
            if not bins >= 1:  # (numpy's message, before any range is looked for)
                raise ValueError("`bins` must be positive, when an integer")
            range = finite_range(0)
        return [_float_edges(np.histogram_bin_edges(np.empty(0), bins, range=range))], (uniform,)
    try:  # np.histogram2d's reading of `bins`
        count = len(bins)
    except TypeError:
        count = 1
    if count != 1 and count != 2:
        bins = [np.asarray(bins), np.asarray(bins)]
    per_axis = [bins, bins] if count == 1 else list(bins)
    if any(isinstance(b, str) for b in per_axis):
        raise ValueError("string bin estimators are not supported: give numbers of bins or the edges")
    ranges = [None, None] if range is None else list(range)
    if len(ranges) != 2:
        raise ValueError("range: a pair of (lo, hi), either of which may be None")
    uniform = tuple(np.ndim(b) == 0 for b in per_axis)
    for axis in (0, 1):
        if uniform[axis] and ranges[axis] is None:
            if not per_axis[axis] >= 1:
                raise ValueError(f"`bins[{axis}]` must be positive, when an integer")
            ranges[axis] = finite_range(axis)
    _, xedges, yedges = np.histogram2d(np.empty(0), np.empty(0), bins=bins, range=ranges)
    return [_float_edges(xedges), _float_edges(yedges)], uniform


def _float_edges(edges):
    return np.ascontiguousarray(edges, dtype=np.float64)  # (the kernel reads float64 edges; integer edges are exact)


def _density(hist, edges):
    """numpy's density normalisation of one histogram (the same operations in the same order)."""
    if len(edges) == 1:
        return hist / np.diff(edges[0]) / hist.sum()
    s = hist.sum()
    hist = hist / np.diff(edges[0]).reshape(-1, 1)
    hist = hist / np.diff(edges[1]).reshape(1, -1)
    hist /= s
    return hist


def _all_reduce_min(tensor, group):
    """Element-wise smallest of a small device tensor over the ranks of a torch.distributed group."""
    import torch.distributed as dist

    if dist.get_backend(group) == "nccl":
        dist.all_reduce(tensor, op=dist.ReduceOp.MIN, group=group)
        return tensor
    host = tensor.cpu()
    dist.all_reduce(host, op=dist.ReduceOp.MIN, group=group)
    return host.to(tensor.device)


def _all_reduce_sum(tensor, group):
    """Sum of a small device tensor over the ranks of a torch.distributed group (through the host for a backend
    that does not take device tensors)."""
    import torch.distributed as dist

    if dist.get_backend(group) == "nccl":
        dist.all_reduce(tensor, group=group)
        return tensor
    host = tensor.cpu()
    dist.all_reduce(host, group=group)
    return host.to(tensor.device)


def _all_reduce_max(value, group, comm, device):
    """Largest of a host number over the ranks (the highest ray id: how many source groups there are)."""
    import torch
    import torch.distributed as dist

    if group is None:  # a bare library communicator: the count is the caller's to give
        raise ValueError("group_stats over a LibraryComm needs n_groups (or pass the torch.distributed group as well)")
    on = device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    box = torch.tensor([value], dtype=torch.float64, device=on)
    dist.all_reduce(box, op=dist.ReduceOp.MAX, group=group)
    return float(box[0])

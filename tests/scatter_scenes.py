"""The scenes of the scatter tests, built on tests/ghost_scenes.py, the models they give their surfaces, and the
reference run: tests/scatter_reference.py on a frame and the snapshot's primitives."""
import numpy as np

import ghost_scenes as gs
import scatter_reference as ref
import scenes

LAMBERT, HARVEY = 0.04, (0.8, 0.02, -1.8)  # albedo; b0, l, s


def stopped_lens(n):
    """A lens behind an aperture stop, a detector, the housing: (parts, rays, detector)."""
    return gs.stopped_lens(n)


def prism(n_per_wavelength):
    return gs.prism(n_per_wavelength)


def two_mirrors(n):
    """Two facing plane mirrors in the housing: every ray lands on a mirror in every generation."""
    parts, rays = scenes.two_mirrors(gs.api(), n)
    return gs.housed(parts), rays, parts[0]


def lens_in_barrel(n):
    """Config 2's lens and detector in the housing, the barrel of the scatter example: (parts, rays, detector)."""
    return gs.lens(n)


def surface_ids(part):
    return [int(sid) for sid, _ in part.surface_ids] if hasattr(part, "surface_ids") else [int(part.get_id())]


def prims_of(parts):
    from pyrayt_amd.scene import SceneSnapshot

    return SceneSnapshot(parts).prims


def tables():
    """(Lambertian, Harvey) as the product tabulates them and as plain arrays for the reference."""
    from pyrayt_amd.scatter import Scatter

    models = (Scatter.lambertian(LAMBERT), Scatter.harvey(*HARVEY))
    return models, np.stack([m.table for m in models])


def split_models(frame, parts):
    """The surfaces the frame's rows land on, in ascending order, alternately Lambertian and Harvey:
    (ids, model number per id)."""
    known = set(int(p["surface_id"]) for p in prims_of(parts))
    met = sorted(set(int(s) for s in np.unique(frame[:, 5]) if s == int(s)) & known)
    return met, [k % 2 for k in range(len(met))]


def product_models(ids, numbers, models):
    """The dict DeviceFrame.scatter takes, the surfaces of a model as one tuple, in the reference's order."""
    out = {}
    for number in sorted(set(numbers), key=numbers.index):
        out[tuple(sid for sid, m in zip(ids, numbers) if m == number)] = models[number]
    order = [sid for key in out for sid in key]
    return out, order, [numbers[ids.index(sid)] for sid in order]


def target_for(det_centre=(1.0, 0.0, 0.0), normal=(1.0, 0.0, 0.0), radius=0.5):
    from pyrayt_amd.scatter import Target

    return Target.disk(det_centre, normal, radius), ref.target_of(det_centre, normal, radius)


def reference(frame, parts, ids, numbers, table_values, **options):
    return ref.scatter(frame, ref.table_of(prims_of(parts)), ids, numbers, table_values, **options)

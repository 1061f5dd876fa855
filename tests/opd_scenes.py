"""Scenes for the wavefront-sensitivity tests, traced on the CPU by the C oracle through tests/design_scenes.py's ``_case``:
each gives the parts, the frame (R, 15), the surface to look at and the parameters.  A builder takes ``change=(k, amount)``
to build the system afresh with parameter k applied by ``amount``, as design_scenes' do.  Rigid motions are written as
``Deformation(part, translate=, rotate=)``, which has the bits of a ``Motion`` in the pass and an ``apply`` besides."""
import numpy as np

import scenes
from design_scenes import _api, _case
from sensitivity_scenes import directed_rays

_CACHE = {}
PLATE = dict(thickness=0.4, index=1.5)
DISH = dict(focus=3.0, beam=0.003)


def build(name, n=257, change=None):
    if change is not None:
        return _BUILDERS[name](n, change)
    if (name, n) not in _CACHE:
        _CACHE[(name, n)] = _BUILDERS[name](n, None)
    return _CACHE[(name, n)]


def _beam(n, x, radius, seed, direction=(1.0, 0.0, 0.0), inner=0.0):
    rng = np.random.default_rng(seed)
    r, angle = radius * np.sqrt(rng.uniform((inner / radius) ** 2, 1.0, n)), rng.uniform(0, 2 * np.pi, n)
    origins = np.column_stack([np.full(n, x), r * np.cos(angle), r * np.sin(angle)])
    return directed_rays(origins, np.tile(direction, (n, 1)))


def detector_move(n, change):
    """A cone onto a detector that is moved along and across the beam: only Q slides along each ray."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    det = c.baffle((4, 4)).move_x(1.0)
    parameters = [Deformation(det, translate=(1, 0, 0)), Deformation(det, translate=(0, 0.3, -0.2)),
                  Deformation(det, rotate=(0, 0, 1), pivot=(1.0, 0.1, 0.0))]
    return _case("detector_move", [det], scenes.cone_rays(n, (-1.0, 0.05, 0.0), 15.0, 61), det, parameters, change)


def plate_square(n, change):
    """A plane-parallel plate square to a collimated beam along x: its index, and its thickness by a stretch along x."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    index = PLATE["index"] + (change[1] if change is not None and change[0] == 0 else 0.0)
    slab = cg.Cuboid.from_sides(PLATE["thickness"], 4, 4, material=matl.BasicRefractor(index)).move(0.5, 0.1, 0)
    det = c.baffle((6, 6)).move_x(3.0)
    return _case("plate_square", [slab, det], _beam(n, -1.0, 0.3, 62), det,
                 [IndexChange(slab), Deformation.stretch(slab, (1, 0, 0))], change, index_changed=True)


def mirror_normal(n, change):
    """A flat mirror at normal incidence, translated along its normal, away from the source."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    mirror = cg.XYPlane(6, 6, material=matl.mirror).rotate_y(-90).move_x(1.0)
    det = c.baffle((4, 4)).move_x(-2.0)
    return _case("mirror_normal", [mirror, det], _beam(n, -1.0, 0.3, 63), det, [Deformation(mirror, translate=(1, 0, 0))],
                 change)


def dish_axial(n, change):
    """A parabolic mirror (focus at the origin) under a collimated axial beam, a ring of it past a small detector in the
    focal plane: the mirror translated along and across its axis.  The beam is slow (NA 1e-3), so that 1 + cos(theta) is
    piston plus defocus to 1e-14."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    dish = c.parabolic_mirror(DISH["focus"], 0.5, aperture=1.5)
    det = c.baffle((0.002, 0.002))
    rays = _beam(n, 2.0, DISH["beam"], 64, direction=(-1.0, 0.0, 0.0), inner=0.0015)
    parameters = [Deformation(dish, translate=(1, 0, 0)), Deformation(dish, translate=(0, 1, 0))]
    return _case("dish_axial", [dish, det], rays, det, parameters, change)


def _lens(index=1.5):
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    glass = c.biconvex_lens(2, 2, 0.25, aperture=1, material=matl.BasicRefractor(index))
    det = c.baffle((1, 1)).move_x(1)
    front = glass.surface_ids[0][1]
    parameters = [Deformation(glass, translate=(0, 1, 0)), Deformation(glass, rotate=(0, 0, 1), pivot=(0, 0, 0)),
                  Deformation.radius(front, keep=(-0.125, 0, 0)), Deformation.stretch(glass, (0, 1, 0)), IndexChange(glass)]
    return glass, det, parameters


def singlet(n, change):
    """The singlet of examples/bend_lens.py (the config-2 lens, a 6 degree cone from its focus: spherical aberration) and
    its detector: a decentre, a tilt, r1 with the vertex kept, a stretch across the axis, the index."""
    glass, det, parameters = _lens(1.5 + (change[1] if change is not None and change[0] == 4 else 0.0))
    rays = scenes.cone_rays(n, (-scenes.lensmakers_equation(2, -2, 1.5, 0.25), 0.0, 0.0), 6.0, 1234)
    return _case("singlet", [glass, det], rays, det, parameters, change, index_changed=True, rays_per_source=None)


def two_fields(n, change):
    """The same lens under two point sources, one on the axis and one off it: two groups of n rays, ids [0, n) and [n, 2 n)."""
    glass, det, parameters = _lens(1.5 + (change[1] if change is not None and change[0] == 4 else 0.0))
    f = scenes.lensmakers_equation(2, -2, 1.5, 0.25)
    a, b = scenes.cone_rays(n, (-f, 0.0, 0.0), 5.0, 65), scenes.cone_rays(n, (-f, 0.12, -0.05), 5.0, 66)
    rays = np.concatenate([a, b], axis=1)
    rays[12] = np.arange(2 * n)
    return _case("two_fields", [glass, det], rays, det, parameters, change, index_changed=True, rays_per_source=n)


_BUILDERS = {f.__name__: f for f in (detector_move, plate_square, mirror_normal, dish_axial, singlet, two_fields)}

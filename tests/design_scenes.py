"""Scenes for the design-sensitivity tests (shape and index parameters), traced on the CPU by the C oracle as
tests/sensitivity_scenes.py does: each gives the parts, the frame (R, 15), the surface to look at and the parameters, a mix
of Motion, Deformation and IndexChange.  Built through pyrayt_amd's own scene objects.  A builder takes ``change=(k,
amount)`` to build the system afresh with parameter k applied by ``amount`` -- through ``Deformation.apply`` itself, or, for
an IndexChange, with a glass of index n + amount: what the central differences of tests/test_host_design_sensitivity.py
trace."""
from types import SimpleNamespace

import numpy as np

import scenes
from sensitivity_scenes import directed_rays, trace

_CACHE = {}


def _api():
    from pyrayt_amd import Deformation, IndexChange, Motion

    api = scenes.product_api()
    return api.cg, api.components, api.materials, Deformation, IndexChange, Motion


def _case(name, parts, rays, surface, parameters, change=None, limit=10, companions=None, **more):
    """companions: {k: function(amount)}, what else the system changed by parameter k needs so that no ray changes its
    path -- a change of a surface that no ray meets, which has no part in the derivative."""
    if change is not None:
        k, amount = change
        if hasattr(parameters[k], "apply"):
            parameters[k].apply(amount)
        else:
            assert more.get("index_changed", False), "the builder puts an IndexChange into the glass itself"
        if companions and k in companions:
            companions[k](amount)
    more.pop("index_changed", None)
    frame, counts = trace(parts, rays, limit)
    return SimpleNamespace(name=name, parts=parts, rays=rays, frame=frame, counts=counts, surface=surface,
                           parameters=parameters, motions=parameters, limit=limit, **more)


def build(name, n=257, change=None):
    """The case ``name`` with n rays (cached: a frame is computed once and shared, never changed); with ``change`` the
    system built afresh and changed, not cached."""
    if change is not None:
        return _BUILDERS[name](n, change)
    key = (name, n)
    if key not in _CACHE:
        _CACHE[key] = _BUILDERS[name](n, None)
    return _CACHE[key]


def _flipped(rays):
    rays = rays.copy()
    rays[4] = -rays[4]
    return rays


# ---- closed forms -------------------------------------------------------------------------------------------------------------
def ball_radius(n, change):
    """A glass ball whose radius grows about its centre, rays aimed at the centre: dx = -d at entry, +d at exit, 0 on the
    detector."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    centre = np.array([0.3, 0.1, -0.05])
    ball = cg.Sphere(0.8, material=matl.glass["BK7"]).move(*centre)
    det = c.baffle((12, 12)).move_x(4.0)
    aim = scenes.cone_rays(n, (0, 0, 0), 30.0, 41)[4:7].T
    return _case("ball_radius", [ball, det], directed_rays(centre - 2.5 * aim, aim), det, [Deformation.radius(ball)], change)


def plane_stretch(n, change):
    """A detector stretched, and sheared, within its own plane: dx = 0."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    det = c.baffle((4, 4)).move_x(1.0).rotate_z(12)
    normal = np.asarray(det.get_orientation(), dtype=float).reshape(-1)[:3]
    t2 = np.array([0.0, 0.0, 1.0])
    t1 = np.cross(t2, normal)
    t1 /= np.linalg.norm(t1)
    shear = 0.7 * np.outer(t1, t1) + 0.2 * np.outer(t1, t2) - 0.4 * np.outer(t2, t1) + 0.3 * np.outer(t2, t2)
    parameters = [Deformation.stretch(det, t1), Deformation(det, linear=shear, pivot=(1.0, 0.2, 0.1))]
    return _case("plane_stretch", [det], scenes.cone_rays(n, (-1.0, 0.0, 0.0), 20.0, 42), det, parameters, change,
                 invariant=True)


def cylinder_stretch(n, change):
    """A mirror cylinder stretched along its own axis and met on its wall: dx = 0."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    rod = cg.Cylinder(0.5, -1.5, 1.5, material=matl.mirror).rotate_x(90).move(0.0, 0.0, 0.2)
    det = c.baffle((12, 12)).move_x(-3.0)
    axis = np.asarray(rod.get_orientation(), dtype=float).reshape(-1)[:3]
    return _case("cylinder_stretch", [rod, det], scenes.cone_rays(n, (-2.0, 0.1, 0.0), 8.0, 43), det,
                 [Deformation.stretch(rod, axis, about=(0.3, -0.4, 0.1))], change, invariant=True)


def similarity(n, change):
    """A glass ball scaled uniformly about the point the rays come from, a point of every ray (the source, scaled with it,
    stays where it is): source and ball go through a similarity, so every direction stays, dd = 0, and a landing point on
    the ball moves with the ball, dx = x - P."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    source = np.array([-2.0, 0.0, 0.0])
    ball = cg.Sphere(0.8, material=matl.glass["BK7"]).move(0.3, 0.1, -0.05)
    det = c.baffle((8, 8)).move_x(4.0)
    return _case("similarity", [ball, det], scenes.cone_rays(n, tuple(source), 12.0, 44), det,
                 [Deformation(ball, linear=np.eye(3), pivot=source)], change, source=source, ball=ball)


PLATE = SimpleNamespace(thickness=0.4, angle=25.0, index=1.5)


def plate(n, change):
    """A tilted plane-parallel plate (a cuboid) in a collimated beam along x: the beam is displaced sideways by
    t sin(a) (1 - cos(a) / sqrt(n^2 - sin(a)^2)), towards +y for a tilt a > 0 about z.  Parameters: the index, and the
    thickness by a stretch along the plate's normal (per unit of relative elongation, t d/dt)."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    index = PLATE.index + (change[1] if change is not None and change[0] == 0 else 0.0)
    slab = cg.Cuboid.from_sides(PLATE.thickness, 4, 4, material=matl.BasicRefractor(index)).rotate_z(PLATE.angle).move(0.5, 0.1, 0)
    det = c.baffle((6, 6)).move_x(3.0)
    normal = np.array([np.cos(np.radians(PLATE.angle)), np.sin(np.radians(PLATE.angle)), 0.0])
    rng = np.random.default_rng(45)
    origins = np.column_stack([np.full(n, -1.0), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)])
    return _case("plate", [slab, det], directed_rays(origins, np.tile([1.0, 0.0, 0.0], (n, 1))), det,
                 [IndexChange(slab), Deformation.stretch(slab, normal)], change, index_changed=True)


def dish_focus(n, change):
    """A parabolic mirror under a collimated axial beam (a ring of it, past a small detector in the focal plane, tilted):
    the focus grows with the vertex kept, the focal point moves by the unit axis e, dx = e - d (e.a) / (d.a)."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    dish = c.parabolic_mirror(3.0, 0.5, aperture=1.5)
    det = c.baffle((0.2, 0.2)).rotate_z(10)
    rng = np.random.default_rng(46)
    radius, angle = rng.uniform(0.3, 0.6, n), rng.uniform(0, 2 * np.pi, n)
    origins = np.column_stack([np.full(n, 2.0), radius * np.cos(angle), radius * np.sin(angle)])
    leaf = dish.surface_ids[1][1]  # (difference(stock, dish): the paraboloid is the right child)
    return _case("dish_focus", [dish, det], directed_rays(origins, np.tile([-1.0, 0.0, 0.0], (n, 1))), det,
                 [Deformation.focus(leaf)], change, axis=np.array([1.0, 0.0, 0.0]))


# ---- systems -------------------------------------------------------------------------------------------------------------------
def lens(n, change):
    """The config-2 lens (a 6 degree cone from the focus, beam radius <= 0.22 in a clear radius of 0.5) and its detector:
    r1 and r2 with the vertices kept, the thickness (the back face pushed along the axis), the index, a decentre.  The
    aperture stock's cap is tangent to the back vertex: in the system changed by the thickness the stock is stretched from
    the front vertex so that it stays so (else a thicker lens has its tip cut off and the rays next to the axis change their
    path); the rays do not meet the stock."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    index = 1.5 + (change[1] if change is not None and change[0] == 3 else 0.0)
    glass = c.biconvex_lens(2, 2, 0.25, aperture=1, material=matl.BasicRefractor(index))
    det = c.baffle((1, 1)).move_x(1)
    front, back = glass.surface_ids[0][1], glass.surface_ids[1][1]
    parameters = [Deformation.radius(front, keep=(-0.125, 0, 0)), Deformation.radius(back, keep=(0.125, 0, 0)),
                  Deformation(back, translate=(1, 0, 0)), IndexChange(glass), Motion(glass, translate=(0, 1, 0))]
    rays = scenes.cone_rays(n, (-scenes.lensmakers_equation(2, -2, 1.5, 0.25), 0.0, 0.0), 6.0, 1234)
    stock = glass.surface_ids[2][1]
    grow = {2: lambda amount: Deformation.stretch(stock, (1, 0, 0), about=(-0.125, 0, 0)).apply(amount / 0.25)}
    return _case("lens", [glass, det], rays, det, parameters, change, index_changed=True, companions=grow)


def mirror(n, change):
    """A concave spherical mirror (c.spherical_mirror) that sends a cone back to a detector: its radius with the vertex
    kept, and about its centre."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    bowl_mirror = c.spherical_mirror(4.0, 0.3, aperture=1.5)
    det = c.baffle((8, 8)).move_x(4.0)
    bowl = bowl_mirror.surface_ids[1][1]  # (difference(stock, bowl))
    parameters = [Deformation.radius(bowl, keep=(0, 0, 0)), Deformation.radius(bowl)]
    return _case("mirror", [bowl_mirror, det], _flipped(scenes.cone_rays(n, (3.0, 0.1, 0.05), 5.0, 47)), det, parameters,
                 change)


def egg(n, change):
    """sensitivity_scenes' `scaled`: a glass ball stretched to an ellipsoid (a minv that is not rigid); its radius, in its
    own frame, about its centre and with a point of its skin kept."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    ball = cg.Sphere(0.7, material=matl.glass["BK7"]).scale(1.0, 1.6, 0.8).rotate_z(25).move(0.2, 0.1, 0.0)
    det = c.baffle((8, 8)).move_x(3.5)
    parameters = [Deformation.radius(ball), Deformation.radius(ball, keep=(-0.6, 0.0, 0.0))]
    return _case("egg", [ball, det], scenes.cone_rays(n, (-2.0, 0.0, 0.0), 8.0, 13), det, parameters, change)


def dish(n, change):
    """A parabolic mirror (components.parabolic_mirror, as in sensitivity_scenes' `paraboloid`) that sends a cone to a
    detector; its focus with the vertex kept, and a tilt.  The cone comes in at 45 degrees to the axis, aimed within 0.3 of
    the vertex (clear radius 0.75): the oracle, like the engine, finds the paraboloid with the textbook quadratic formula,
    whose wanted root cancels for a ray along the axis (absolute error of t about eps * 4 f / (2 |d_perp|^2)); at 45
    degrees that is the few eps of the landing point that the rounding floor of the central differences assumes, at 5
    degrees it is fifty times as much."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    glass = c.parabolic_mirror(3.0, 0.5, aperture=1.5)
    det = c.baffle((12, 12)).move_x(1.0)
    parameters = [Deformation.focus(glass.surface_ids[1][1]), Motion(glass, rotate=(0, 0, 1))]
    rng = np.random.default_rng(48)
    radius, angle = 0.3 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    targets = np.column_stack([np.full(n, -3.0), radius * np.cos(angle), radius * np.sin(angle)])
    origin = np.array([-1.0, 2.0, 0.1])
    return _case("dish", [glass, det], directed_rays(np.tile(origin, (n, 1)), targets - origin), det, parameters, change)


def stopped(n, change):
    """sensitivity_scenes' `stopped`: a stop that absorbs part of the beam in mid-path (rays end early, their id slots go
    stale), a plano-convex lens of SF2, a detector: the radius of the lens's sphere with its vertex kept, the index, a
    shift of the stop."""
    cg, c, matl, Deformation, IndexChange, Motion = _api()
    parts, rays = scenes.stopped_lens(scenes.product_api(), n)
    stop, glass, det = parts
    sphere = glass.surface_ids[0][1]  # (intersect(face, stock))
    parameters = [Deformation.radius(sphere, keep=(0.15, 0, 0)), IndexChange(glass), Motion(stop, translate=(1, 0, 0))]
    return _case("stopped", parts, rays, det, parameters, change)


_BUILDERS = {f.__name__: f for f in (ball_radius, plane_stretch, cylinder_stretch, similarity, plate, dish_focus, lens,
                                     mirror, egg, dish, stopped)}
CLOSED_FORMS = ("ball_radius", "plane_stretch", "cylinder_stretch", "similarity", "plate", "dish_focus")
SYSTEMS = ("lens", "mirror", "egg", "dish", "stopped")
# (system, parameter) pairs that the central differences of the oracle check
DIFFERENCED = (("lens", 0), ("lens", 1), ("lens", 2), ("lens", 3), ("mirror", 0), ("egg", 0), ("dish", 0))

"""The host side of the scatter pass (CPU): the numpy restatement of the definitions (tests/scatter_reference.py) --
Philox against the published known-answer vectors, the exact fused multiply-add behind the surface normal against
rational arithmetic, the samples, the basis, the table look-up, the fates, the stable order -- its energy balance in both
modes against closed forms, the Scatter models, the refusals that come before any GPU call, and the ABI."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import fresnel_reference as fref
import scatter_reference as ref

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IX = fref.IX
PLATE = {7: (ref.PLANE, 1, np.zeros(6), np.eye(4).reshape(16))}  # the plane z = 0, normal +z


def plate_frame(n, direction=(0.0, 0.0, -1.0), surface=7, generation=0):
    """n rows of intensity 1 that land on the origin of the plate along `direction`."""
    frame = np.zeros((n, 15))
    frame[:, IX["id"]], frame[:, IX["generation"]] = np.arange(n), generation
    frame[:, IX["intensity"]], frame[:, IX["wavelength"]], frame[:, IX["index"]] = 1.0, 0.55, 1.0
    frame[:, IX["surface"]], frame[:, 12:15] = surface, direction
    return frame


def lambert(albedo):
    return np.full((1, ref.KNOTS + 1), albedo / np.pi)


# ---- random numbers -----------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """The three vectors of the Random123 distribution's kat_vectors for philox4x32 with 10 rounds."""
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in cases:
        got = ref.philox(np.array([counter], dtype=np.uint64), key)[0]
        assert " ".join(f"{int(v):08x}" for v in got) == want


def test_uniforms_lie_in_the_half_open_unit_interval_and_depend_on_the_counter_alone():
    top = np.uint64(0xffffffff)
    assert ref.uniform(top, top) == 1.0 - 2.0 ** -53 and ref.uniform(np.uint64(0), np.uint64(0)) == 0.0
    assert ref.uniform(np.uint64(0), np.uint64(2047)) == 0.0 and ref.uniform(np.uint64(0), np.uint64(2048)) == 2.0 ** -53
    ids = np.arange(5000) + 2 ** 33  # (the high word of the id counts)
    a, b = ref.samples(ids, np.full(5000, 3), np.arange(5000) % 7, seed=2 ** 40 + 5)
    assert np.all((a >= -1) & (a < 1) & (b >= -1) & (b < 1)) and abs(a.mean()) < 0.05 and abs(b.mean()) < 0.05
    order = np.random.default_rng(0).permutation(5000)
    a2, b2 = ref.samples(ids[order], np.full(5000, 3), (np.arange(5000) % 7)[order], seed=2 ** 40 + 5)
    assert np.array_equal(a2, a[order]) and np.array_equal(b2, b[order])
    low, _ = ref.samples(ids - 2 ** 33, np.full(5000, 3), np.arange(5000) % 7, seed=2 ** 40 + 5)
    other, _ = ref.samples(ids, np.full(5000, 3), np.arange(5000) % 7, seed=5)
    assert not np.array_equal(low, a) and not np.array_equal(other, a)


def test_the_fused_multiply_add_is_exact():
    rng = np.random.default_rng(1)
    n = 3000
    a, b, c = (rng.normal(size=n) * 10.0 ** rng.integers(-6, 6, n) for _ in range(3))
    c[:1000] = -(a[:1000] * b[:1000])  # (cancellation: the result is the product's rounding error)
    c[1000:1500] = np.nextafter(-(a[1000:1500] * b[1000:1500]), np.inf)
    a[1500:1600], c[1600:1700] = 0.0, 0.0
    a[1700:2300] = 1.0 + rng.integers(0, 2 ** 26, 600) * 2.0 ** -26  # (exact products and a far smaller c: the ties)
    b[1700:2300] = 1.0 + rng.integers(0, 2 ** 26, 600) * 2.0 ** -26
    c[1700:2300] = rng.choice([1.0, -1.0], 600) * 2.0 ** -rng.integers(50, 110, 600).astype(float)
    got = ref.fma(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        want = float(exact)  # (int / int division of Fraction.__float__ rounds correctly)
        assert g == want, (x, y, z)
    assert np.signbit(ref.fma(-0.0, 1.0, -0.0)) and not np.signbit(ref.fma(0.0, 1.0, -0.0))  # (as IEEE adds zeros)


# ---- geometry -------------------------------------------------------------------------------------------------------------
def test_the_basis_is_orthonormal_near_the_poles_and_the_axes():
    rng = np.random.default_rng(2)
    tiny = [0.0, 1e-300, 1e-17, 1e-9, 1e-3]
    normals = [(s * e, -e, z * np.sqrt(1 - 2 * e * e)) for e in tiny for z in (1.0, -1.0) for s in (1.0, -1.0)]
    normals += [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 0, -0.0), (0, -1, -0.0)]
    normals += list(ref.unit(rng.normal(size=(3, 200))).T)
    n = ref.unit(np.array(normals, dtype=float).T)
    t1, t2 = ref.basis(n)
    eps = np.finfo(float).eps
    for u, v, want in ((t1, t1, 1), (t2, t2, 1), (n, n, 1), (t1, t2, 0), (t1, n, 0), (t2, n, 0)):
        assert np.all(np.abs(ref.dot(u, v) - want) <= 8 * eps)
    cross = np.cross(t1.T, t2.T).T  # (right-handed: t1 x t2 = n)
    assert np.all(np.abs(cross - n) <= 8 * eps)
    from pyrayt_amd.scatter import basis

    for k in range(0, n.shape[1], 17):
        e1, e2 = basis(n[:, k])
        assert np.array_equal(e1, t1[:, k]) and np.array_equal(e2, t2[:, k])


def test_world_normals_of_the_five_primitives():
    """Against the longdouble normals of tests/sensitivity_reference.py, to a few ulp; unit length; the scale's sign."""
    import sensitivity_reference as sref

    rng = np.random.default_rng(3)
    angle = 0.3
    rotation = np.array([[np.cos(angle), -np.sin(angle), 0, 0.4], [np.sin(angle), np.cos(angle), 0, -0.2], [0, 0, 1, 0.1],
                         [0, 0, 0, 1.0]])
    cases = {ref.SPHERE: ((1.5, 0, 0, 0, 0, 0), lambda u: 1.5 * u),
             ref.CYLINDER: ((0.7, -1, 1, 0, 0, 0), lambda u: np.stack([0.7 * u[0] / np.hypot(u[0], u[1]), 0.7 * u[1] / np.hypot(u[0], u[1]), 0.5 * u[2]])),
             ref.PLANE: ((2, 2, 0, 0, 0, 0), lambda u: np.stack([u[0], u[1], 0 * u[2]])),
             ref.CUBE: ((-1, 1, -1, 1, -1, 1), lambda u: np.stack([0.5 * u[0], 0.5 * u[1], np.ones_like(u[2])])),
             ref.PARABOLOID: ((0.5, 1.5, 0, 0, 0, 0), lambda u: np.stack([u[0], u[1], (u[0] ** 2 + u[1] ** 2) / 2.0]))}
    for kind, (params, on) in cases.items():
        local = on(ref.unit(rng.normal(size=(3, 64))))
        world = (np.linalg.inv(rotation) @ np.vstack([local, np.ones(64)]))[:3]
        for scale in (1, -1):
            entry = (kind, scale, np.array(params, dtype=float), rotation.reshape(16))
            got = ref.world_normal(entry, world)
            want, _ = sref.surface_normals((kind, scale, entry[2], rotation), world.T.astype(np.longdouble),
                                           -got.T.astype(np.longdouble))  # (d against n: no flip)
            assert np.all(np.abs(got.T - want.astype(float)) <= 1e-9), kind  # (points rounded onto the surface)
            assert np.all(np.abs(ref.dot(got, got) - 1) <= 8 * np.finfo(float).eps)
    edge = ref.world_normal((ref.CUBE, 1, np.array([-1, 1, -1, 1, -1, 1.0]), np.eye(4).reshape(16)), np.array([[0.3], [0.2], [0.1]]))
    assert np.all(np.isnan(edge))  # (a point on no face: 0 / 0, as upstream)


def test_the_table_lookup():
    from pyrayt_amd.scatter import KNOTS, Scatter, knots

    assert KNOTS == ref.KNOTS and knots()[0] == 0.0 and knots()[-1] == 2.0 and abs(knots()[1] - 2.0 / KNOTS ** 2) < 1e-20
    model = Scatter.harvey(0.8, 0.02, -1.8)
    b = np.concatenate([knots(), [1e-300, 1e-9, 0.3, 1.999999, 2.0, 2.0000001, 2.5], np.random.default_rng(4).uniform(0, 2, 500)])
    got = ref.lookup(model.table, b)
    assert np.array_equal(got, model.lookup(b))
    at_knots = got[:KNOTS + 1]
    assert np.all(np.abs(at_knots - model.table) <= 1e-9 * model.table)  # (sqrt(b / 2) * T lands within an ulp of k)
    inside = b <= 2.0  # (past 2 the last interval is extended)
    assert np.all((got[inside] >= model.table.min() * (1 - 1e-12)) & (got[inside] <= model.table.max()))
    assert np.all(np.isnan(ref.lookup(model.table, np.array([np.nan, -1.0]))))
    exact = 0.8 * (1 + (b[-500:] / 0.02) ** 2) ** -0.9
    assert np.all(np.abs(got[-500:] - exact) <= 1.01 * model.table_error() * exact)  # (worst at a midpoint)


# ---- the Scatter models ------------------------------------------------------------------------------------------------------
def test_scatter_models():
    from pyrayt_amd.scatter import Scatter

    plain = Scatter.lambertian(0.3)
    assert plain.table_error() == 0 and plain.tis() == 0.3 and plain.tis(0.9) == 0.3
    assert np.all(plain.table == 0.3 / np.pi) and plain.kind == "lambertian" and plain.parameters == dict(albedo=0.3)
    by_quadrature = Scatter.from_callable(lambda b: np.full(np.shape(b), 0.3 / np.pi))
    for theta in (0.0, 0.5, 1.2):  # (the integral of a constant over the unit disk, from any point of it)
        assert abs(by_quadrature.tis(theta) - 0.3) < 1e-12
    # Harvey-Shack with s = -2 at normal incidence: 2 pi b0 int_0^1 r / (1 + (r/l)^2) dr = pi b0 l^2 ln(1 + 1/l^2)
    b0, l = 0.5, 0.05
    wing = Scatter.harvey(b0, l, -2.0)
    assert abs(wing.tis() - np.pi * b0 * l * l * np.log1p(1 / (l * l))) < 1e-9
    assert 0 < wing.table_error() < 1e-3 and wing.table[0] == b0
    # ABg with g = 2 is the same family: a / (b + beta^2) = (a / b) / (1 + (beta / sqrt(b))^2)
    abg = Scatter.abg(b0 * l * l, l * l, 2.0)
    assert np.allclose(abg.table, wing.table, rtol=1e-13) and abs(abg.tis() - wing.tis()) < 1e-12
    measured = Scatter.tabulated([0.0, 0.5, 2.0], [1.0, 0.5, 0.2])
    assert measured.table[0] == 1.0 and measured.table[-1] == 0.2 and abs(measured.lookup(np.array([0.25]))[0] - 0.75) < 1e-3
    for bad in (lambda: Scatter.lambertian(1.5), lambda: Scatter.harvey(1, 0, -1), lambda: Scatter.abg(1, 0, 2),
                lambda: Scatter.tabulated([0, 0], [1, 1]), lambda: Scatter.from_callable(lambda b: -1 + 0 * b),
                lambda: Scatter.from_callable(lambda b: 1 / b)):
        with pytest.raises(ValueError):
            bad()


def test_target_disk():
    from pyrayt_amd.scatter import Target

    disk = Target.disk((1, 2, 3), (0, 0, -2), 0.5)
    assert np.array_equal(disk.packed(), ref.target_of((1, 2, 3), (0, 0, -2), 0.5)) and disk.packed().shape == (13,)
    assert np.array_equal(disk.normal, (0, 0, -1)) and abs(np.dot(disk.e1, disk.e2)) == 0
    for bad in (lambda: Target.disk((0, 0, 0), (0, 0, 0), 1), lambda: Target.disk((0, 0, 0), (0, 0, 1), 0),
                lambda: Target.disk((0, 0), (0, 0, 1), 1), lambda: Target.disk((0, 0, np.inf), (0, 0, 1), 1)):
        with pytest.raises(ValueError):
            bad()


# ---- fates, order, invariance ---------------------------------------------------------------------------------------------
def test_buckets_groups_ids_and_the_stable_order():
    frame = np.concatenate([plate_frame(30, surface=7), plate_frame(30, surface=3, generation=1), plate_frame(30, surface=9, generation=2)])
    frame[30:60, IX["id"]], frame[60:, IX["id"]] = np.arange(30), np.arange(30)
    frame[:, 12:15] = ref.unit(np.random.default_rng(5).normal(size=(3, 90)) - np.array([[0], [0], [3.0]])).T
    table = {**PLATE, 3: PLATE[7], 5: PLATE[7]}
    tables = np.concatenate([lambert(0.3), lambert(0.6)])
    got = ref.scatter(frame, table, [3, 5, 7], [0, 1, 1], tables, rays_per_hit=3, seed=9, rays_per_group=8, n_groups=4)
    a, b = ref.samples(np.repeat(frame[:60, IX["id"]], 3), np.repeat(frame[:60, IX["generation"]], 3), np.tile(np.arange(3), 60), 9)
    accepted = (a * a + b * b) < 1.0
    items = [(int(frame[p, IX["id"]] // 8) * 3 + (2 if p < 30 else 0), p, c) for p in range(60) for c in range(3) if accepted[3 * p + c]]
    items.sort()
    assert got["parent_row"].tolist() == [p for _, p, _ in items] and got["child"].tolist() == [c for _, _, c in items]
    counts = np.bincount([k for k, _, _ in items], minlength=12)
    assert got["counts"].tolist() == counts.tolist() and got["stride"] == counts.max() and got["n_groups"] == 8
    assert got["keys"].tolist() == [[k // 3, [3, 5, 7][k % 3]] for k in np.flatnonzero(counts)]
    ids = [group * counts.max() + rank for group, k in enumerate(np.flatnonzero(counts)) for rank in range(counts[k])]
    assert got["rays"][12].tolist() == ids
    assert (got["n_spawned"], got["n_rejected"]) == (len(items), 180 - len(items)) and got["n_dark"] == got["n_invalid"] == 0
    on_7 = got["parent_row"] < 30  # (model 1 on surface 7: twice the energy of model 0 on surface 3, bit for bit)
    assert np.all(got["rays"][9][on_7] == 4.0 * (0.6 / np.pi) / 3) and np.all(got["rays"][9][~on_7] == 4.0 * (0.3 / np.pi) / 3)
    assert np.all(got["rays"][6] > 0) and np.all(got["rays"][8] == 0) and np.all(got["rays"][3] == 1)
    # the reference refuses what the definitions refuse
    with pytest.raises(ValueError, match="not below n_groups"):
        ref.scatter(frame, table, [3, 7], [0, 1], tables, rays_per_group=8, n_groups=3)
    bad = frame.copy()
    bad[3, IX["id"]] = 2.5
    with pytest.raises(ValueError, match="not an integer"):
        ref.scatter(bad, table, [7], [0], tables)
    with pytest.raises(ValueError, match="not in the surface table"):
        ref.scatter(frame, table, [8], [0], tables)


def test_fates():
    frame = plate_frame(200)
    accepted = ref.scatter(frame, PLATE, [7], [0], lambert(0.3), rays_per_hit=2)["n_spawned"]
    behind = ref.scatter(frame, PLATE, [7], [0], lambert(0.3), target=ref.target_of((0, 0, -1), (0, 0, 1), 0.5), rays_per_hit=2)
    assert behind["n_below"] == accepted and behind["n_spawned"] == 0 and behind["n_rejected"] == 400 - accepted
    dark = ref.scatter(frame, PLATE, [7], [0], lambert(0.0), rays_per_hit=2)
    assert dark["n_dark"] == accepted and dark["n_spawned"] == 0 and dark["rays"].shape == (13, 0)
    median = float(np.median(ref.scatter(frame, PLATE, [7], [0], np.linspace(1, 2, 1025)[None], rays_per_hit=2)["rays"][9]))
    some = ref.scatter(frame, PLATE, [7], [0], np.linspace(1, 2, 1025)[None], rays_per_hit=2, min_intensity=median)
    assert some["n_dropped"] + some["n_spawned"] == accepted and abs(some["n_dropped"] - accepted / 2) <= 1
    cube = {7: (ref.CUBE, 1, np.array([-1, 1, -1, 1, -1, 1.0]), np.eye(4).reshape(16))}
    inside = ref.scatter(frame, cube, [7], [0], lambert(0.3), rays_per_hit=2)  # (the origin lies on no face)
    assert inside["n_invalid"] == accepted and inside["n_spawned"] == 0
    inside = ref.scatter(frame, cube, [7], [0], lambert(0.3), target=ref.target_of((0, 0, 1), (0, 0, 1), 0.5), rays_per_hit=2)
    assert inside["n_invalid"] == accepted
    still = plate_frame(50, direction=(0.0, 0.0, 0.0))
    assert ref.scatter(still, PLATE, [7], [0], lambert(0.3))["n_spawned"] == 0
    empty = ref.scatter(np.zeros((0, 15)), PLATE, [7], [0], lambert(0.3))
    assert empty["rays"].shape == (13, 0) and empty["n_groups"] == 0 and empty["stride"] == 0


def test_a_child_depends_on_its_row_and_its_number_alone():
    frame = plate_frame(300, direction=(0.3, -0.2, -1.0))
    frame[:, 9:12] = np.random.default_rng(6).normal(size=(300, 3)) * (1, 1, 0)
    harvey = 0.8 * (1 + (2 * (np.arange(1025) / 1024) ** 2 / 0.02) ** 2) ** -0.9
    for target in (None, ref.target_of((0.2, 0.1, 2.0), (0.1, 0, -1), 0.7)):
        one = ref.scatter(frame, PLATE, [7], [0], harvey[None], target=target, rays_per_hit=1, seed=3)
        four = ref.scatter(frame, PLATE, [7], [0], harvey[None], target=target, rays_per_hit=4, seed=3)
        first = four["child"] == 0
        assert np.array_equal(four["parent_row"][first], one["parent_row"])
        assert np.array_equal(four["rays"][:9, first], one["rays"][:9])
        assert np.array_equal(4.0 * four["rays"][9, first], one["rays"][9]) and len(one["parent_row"]) > 200
        order = np.random.default_rng(7).permutation(300)
        shuffled = ref.scatter(frame[order], PLATE, [7], [0], harvey[None], target=target, rays_per_hit=4, seed=3)

        def lines(result, rows):
            keys = np.stack([rows[result["parent_row"], IX["id"]], result["child"].astype(float)])
            table = np.concatenate([keys, result["rays"][:12]]).T
            return table[np.lexsort(keys[::-1])]

        assert np.array_equal(lines(shuffled, frame[order]), lines(four, frame))


# ---- energy balance against closed forms ---------------------------------------------------------------------------------------
# The sum of the children's energies per unit of incoming energy is an unbiased estimate; its standard error comes from the
# children's own energies (scatter_reference.estimate).  Held to 5 standard errors at the sizes and seeds written here.
@pytest.mark.parametrize("rows, rays_per_hit, seed", [(4096, 4, 0), (1500, 16, 1), (20000, 1, 2 ** 63 + 11)])
def test_the_lambertian_hemisphere_returns_the_albedo(rows, rays_per_hit, seed):
    got = ref.scatter(plate_frame(rows, direction=(0.5, 0.1, -1.0)), PLATE, [7], [0], lambert(0.3), rays_per_hit=rays_per_hit, seed=seed)
    total, sigma = ref.estimate(got["rays"][9], rows, rays_per_hit)
    print(f"hemisphere {rows} x {rays_per_hit}, seed {seed}: {total:.6f} +- {sigma:.6f}: {(total - 0.3) / sigma:+.2f} standard errors")
    assert abs(total - 0.3) <= 5 * sigma and sigma < 0.01
    mean_z = float(np.mean(got["rays"][6]))  # (cosine-weighted: the mean of cos is 2 / 3, its standard deviation sqrt(1 / 18))
    assert abs(mean_z - 2 / 3) <= 5 * np.sqrt(1 / 18 / got["n_spawned"])


@pytest.mark.parametrize("rows, rays_per_hit, seed", [(4096, 4, 0), (1500, 16, 1), (20000, 1, 2 ** 63 + 11)])
def test_the_transfer_to_a_coaxial_disk(rows, rays_per_hit, seed):
    """A Lambertian point at the origin sends rho R^2 / (R^2 + d^2) into a coaxial disk of radius R at distance d."""
    radius, distance = 0.5, 1.0
    target = ref.target_of((0, 0, distance), (0, 0, 1), radius)
    got = ref.scatter(plate_frame(rows), PLATE, [7], [0], lambert(0.3), target=target, rays_per_hit=rays_per_hit, seed=seed)
    total, sigma = ref.estimate(got["rays"][9], rows, rays_per_hit)
    exact = 0.3 * radius ** 2 / (radius ** 2 + distance ** 2)
    print(f"disk {rows} x {rays_per_hit}, seed {seed}: {total:.6f} +- {sigma:.6f}: {(total - exact) / sigma:+.2f} standard errors")
    assert abs(total - exact) <= 5 * sigma and sigma < 0.002
    landing = got["rays"][0:3] + got["rays"][4:7] * ((distance - got["rays"][2]) / got["rays"][6])
    assert np.all(np.hypot(landing[0], landing[1]) <= radius * (1 + 1e-12))


def test_both_modes_agree_on_a_harvey_surface_seen_obliquely():
    """No closed form: the disk mode's estimate of the energy into the disk against the hemisphere mode's children that
    fly through the same disk, each with its own standard error."""
    rows, n = 6000, 8
    frame = plate_frame(rows, direction=(0.4, 0.0, -1.0))
    table = (0.05 * (1 + (2 * (np.arange(1025) / 1024) ** 2 / 0.3) ** 2) ** -0.75)[None]
    centre, radius = np.array([0.5, 0.0, 1.0]), 0.6
    toward = ref.scatter(frame, PLATE, [7], [0], table, target=ref.target_of(centre, (0, 0, 1), radius), rays_per_hit=n, seed=4)
    aimed, sigma_aimed = ref.estimate(toward["rays"][9], rows, n)
    wide = ref.scatter(frame, PLATE, [7], [0], table, rays_per_hit=n, seed=5)
    reach = wide["rays"][0:3] + wide["rays"][4:7] * ((centre[2] - wide["rays"][2]) / wide["rays"][6])
    through = np.hypot(reach[0] - centre[0], reach[1] - centre[1]) <= radius
    found, sigma_found = ref.estimate(wide["rays"][9][through], rows, n)
    print(f"disk mode {aimed:.6f} +- {sigma_aimed:.6f}, hemisphere mode {found:.6f} +- {sigma_found:.6f}")
    assert abs(aimed - found) <= 5 * np.hypot(sigma_aimed, sigma_found) and sigma_aimed < 0.5 * sigma_found


# ---- refusals, before any GPU call ----------------------------------------------------------------------------------------------
def host_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist()
    return DeviceFrame(torch.from_numpy(np.ascontiguousarray(frame.T)), counts)


def test_what_the_pass_refuses_before_it_reaches_the_library(monkeypatch):
    import pyrayt_amd as pyrayt
    from pyrayt_amd import engine, scatter
    from pyrayt_amd.scatter import Scatter, Target

    monkeypatch.setattr(engine, "library", lambda: pytest.fail("the library was reached"))
    pyrayt.g3d.objects.CountedObject.reset_ids()
    wall = pyrayt.components.baffle((1, 1))
    sid = wall.get_id()
    device = host_frame(plate_frame(20, surface=sid))
    model = Scatter.lambertian(0.1)
    with pytest.raises(ValueError, match="models is a dict"):
        device.scatter([sid], [wall])
    with pytest.raises(ValueError, match="not a Scatter"):
        device.scatter({sid: 0.1}, [wall])
    with pytest.raises(ValueError, match="two models"):
        device.scatter({sid: model, wall: Scatter.lambertian(0.2)}, [wall])
    with pytest.raises(ValueError, match="at most 64 surfaces"):
        device.scatter({tuple(range(65)): model}, [wall])
    with pytest.raises(ValueError, match="at most 16 models"):
        device.scatter({k: Scatter.lambertian(0.01 * k) for k in range(17)}, [wall])
    with pytest.raises(ValueError, match="toward is None"):
        device.scatter({sid: model}, [wall], toward=(0, 0, 1))
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="rays_per_hit"):
            device.scatter({sid: model}, [wall], rays_per_hit=bad)
    for bad in (-1, 2 ** 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            device.scatter({sid: model}, [wall], seed=bad)
    with pytest.raises(ValueError, match="min_intensity"):
        device.scatter({sid: model}, [wall], min_intensity=-1.0)
    with pytest.raises(ValueError, match="system="):
        device.scatter({sid: model}, None)
    with pytest.raises(ValueError, match="not in system"):
        device.scatter({sid + 50: model}, [wall])
    with pytest.raises(ValueError, match="at most 65535 buckets"):
        device.scatter({sid: model}, [wall], rays_per_source=1, n_groups=65536)
    with pytest.raises(ValueError, match="without the column"):
        from pyrayt_amd.frame import DeviceFrame

        DeviceFrame(torch.zeros((15, 2), dtype=torch.float64), [2], columns=(0, 1, 4, 5)).scatter({sid: model}, [wall])
    with pytest.raises(pytest.fail.Exception, match="the library was reached"):  # (a good call passes the checks)
        device.scatter({sid: model}, [wall], toward=Target.disk((0, 0, 1), (0, 0, 1), 0.5), rays_per_hit=64, seed=2 ** 64 - 1)
    assert (scatter.KNOTS, scatter.MAX_MODELS, scatter.MAX_SURFACES, scatter.MAX_BUCKETS, scatter.MAX_RAYS_PER_HIT) == \
        (ref.KNOTS, ref.MAX_MODELS, ref.MAX_SURFACES, ref.MAX_BUCKETS, ref.MAX_RAYS_PER_HIT)


def test_the_library_refuses_everything_before_a_device_is_touched():
    from pyrayt_amd import engine
    from pyrayt_amd.scene import PRIM_DTYPE

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    prims = np.zeros(3, dtype=PRIM_DTYPE)
    prims["type"], prims["normal_scale"], prims["surface_id"] = ref.PLANE, 1, (2, 5, 9)
    prims["minv"] = np.eye(4).reshape(16)
    rows = np.zeros((15, 8))
    good = dict(rows=rows.ctypes.data, ld=8, n_rows=8, prims=prims, n_prims=3, surfaces=np.array([5, 2], dtype=np.int64),
                models=np.array([0, 1], dtype=np.int32), n_surfaces=2, tables=np.ones((2, 1025)), n_models=2,
                target=ref.target_of((0, 0, 1), (0, 0, 1), 0.5), rays_per_hit=4, seed=1, rays_per_group=4.0, n_groups=2,
                min_intensity=0.0, ray_offset=1e-6)
    counts, record, work = np.zeros(65535, dtype=np.int64), np.zeros(8, dtype=np.int64), np.zeros(1024)

    def call(**change):
        a = {**good, **change}
        pointer = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v  # noqa: E731
        rc = lib.prt_frame_scatter_count(-7, a["rows"], a["ld"], a["n_rows"], pointer(a["prims"]), a["n_prims"],
                                         pointer(a["surfaces"]), pointer(a["models"]), a["n_surfaces"], pointer(a["tables"]),
                                         a["n_models"], pointer(a["target"]), a["rays_per_hit"], a["seed"], a["rays_per_group"],
                                         a["n_groups"], a["min_intensity"], a["ray_offset"], counts.ctypes.data,
                                         record.ctypes.data, work.ctypes.data, None)
        return rc, lib.prt_last_error().decode()

    unsorted = prims[[1, 0, 2]].copy()
    twice = prims.copy()
    twice["surface_id"] = (2, 2, 9)
    odd = prims.copy()
    odd["type"][1] = 9
    bad_tables = [np.full((2, 1025), v) for v in (-1e-300, np.inf, np.nan)]
    tilted = good["target"].copy()
    tilted[3:6] = (0, 0, 1 + 1e-9)
    flat, endless = good["target"].copy(), good["target"].copy()
    flat[12], endless[0] = 0.0, np.inf
    refused = [(dict(rays_per_hit=0), "1 to 64 rays"), (dict(rays_per_hit=65), "1 to 64 rays"),
               (dict(n_rows=2 ** 29, ld=2 ** 29), "below 2\\^31"), (dict(ld=7), "bad buffers"), (dict(n_surfaces=0), "1 to 64 surfaces"),
               (dict(n_surfaces=65), "1 to 64 surfaces"), (dict(n_models=0), "1 to 16 models"), (dict(n_models=17), "1 to 16 models"),
               (dict(n_groups=32768), "65535"), (dict(rays_per_group=0.0), "one group"), (dict(min_intensity=-1.0), "min_intensity"),
               (dict(ray_offset=np.inf), "ray_offset"), (dict(prims=unsorted), "sorted by id"), (dict(prims=twice), "sorted by id"),
               (dict(prims=odd), "unknown kind"), (dict(surfaces=np.array([5, 5], dtype=np.int64)), "listed twice"),
               (dict(surfaces=np.array([5, 3], dtype=np.int64)), "not in the surface table"),
               (dict(models=np.array([0, 2], dtype=np.int32)), "model is not in"),
               (dict(target=tilted), "unit vector"), (dict(target=flat), "radius is > 0"), (dict(target=endless), "target is finite")]
    refused += [(dict(tables=t), "finite and >= 0") for t in bad_tables]
    for change, message in refused:
        rc, said = call(**change)
        assert rc == -1 and re.search(message, said), (change.keys(), said)
    rc, said = call()  # (what is left is the device, which -7 is not)
    assert rc != 0 and rc != -1 or "device" in said
    assert call(n_rows=0)[0] == 0 and call(n_rows=0, target=None)[0] == 0  # (an empty frame needs no device)
    sizes = lib.prt_frame_scatter_count_workspace_bytes
    assert sizes(1000, 4, 8, 2) > 4000 * 4 + 2 * 1025 * 8 and sizes(1000, 4, 8, 2) < sizes(1000, 5, 8, 2) < sizes(1000, 5, 8, 3)
    for bad in ((-1, 4, 8, 2), (1000, 0, 8, 2), (1000, 65, 8, 2), (2 ** 29, 4, 8, 2), (1000, 4, 0, 2), (1000, 4, 65536, 2), (1000, 4, 8, 0), (1000, 4, 8, 17)):
        assert sizes(*bad) == -1, bad
    assert lib.prt_frame_scatter_emit_workspace_bytes(1000, 4, 8) > 0 and lib.prt_frame_scatter_emit_workspace_bytes(1000, 65, 8) == -1
    assert lib.prt_frame_scatter_emit(-7, rows.ctypes.data, 8, 8, 4, 4, 2, 0, None, None, 0, None, None, work.ctypes.data, None) == -1
    assert lib.prt_frame_scatter_emit(-7, rows.ctypes.data, 8, 0, 4, 4, 2, 3, work.ctypes.data, work.ctypes.data, 8,
                                      work.ctypes.data, work.ctypes.data, work.ctypes.data, None) == -1  # (no rows, children)


# ---- the ABI and the layers ------------------------------------------------------------------------------------------------------
def test_the_header_and_the_binding_agree():
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64}
    names = ["prt_frame_scatter_count", "prt_frame_scatter_count_workspace_bytes", "prt_frame_scatter_emit",
             "prt_frame_scatter_emit_workspace_bytes"]
    for name in names:
        result, arguments = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text).groups()
        wanted = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in arguments.split(",")]
        assert engine.SIGNATURES[name] == (kinds[result], wanted), name
        assert name in engine.EXPORTED_SYMBOLS
    assert engine.PRT_VERSION == 240 and "#define PRT_VERSION 240" in header
    assert "prt_frame_scatter_count" in re.search(r"#define PRT_VERSION \d+ /\*(.*?)\*/", header, flags=re.S).group(1)
    for stated in ("Philox4x32-10", "D2511F53", "copysign", "q = sqrt(0.5 b) * 1024.0", "((4.0 I) f) / N", "cos_o <= 0"):
        assert stated in header, stated
    if os.path.exists(engine.LIB_PATH):
        lib = ctypes.CDLL(engine.LIB_PATH)
        assert all(hasattr(lib, name) for name in names)


def test_frame_and_tracer_only_delegate():
    frame = open(os.path.join(ROOT, "pyrayt_amd", "frame.py")).read()
    tracer = open(os.path.join(ROOT, "pyrayt_amd", "tracer.py")).read()
    module = open(os.path.join(ROOT, "pyrayt_amd", "scatter.py")).read()
    assert "prt_frame_scatter" not in frame and "scatter.spawn(self" in frame
    assert "scatter.trace_scatter(self" in tracer and "prt_frame_scatter" not in tracer
    assert "prt_frame_scatter_count" in module and "prt_frame_scatter_emit" in module
    import pyrayt_amd as pyrayt
    from pyrayt_amd.ghosts import GhostRays

    assert issubclass(pyrayt.scatter.ScatterRays, GhostRays) and "scatter" in pyrayt.__all__
    kernels = open(os.path.join(ROOT, "pyrayt_amd", "csrc", "prt_scatter.hpp")).read()
    for shared in ("k_ghost_tally", "k_sort_offsets", "k_ghost_groups", "fresnel_count", "world_normal_len"):
        assert shared in kernels
    assert "atomicAdd(" not in kernels and "prt_scatter.hpp" in open(os.path.join(ROOT, "pyrayt_amd", "csrc", "Makefile")).read()

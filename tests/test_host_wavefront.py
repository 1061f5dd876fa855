"""The host side of the wavefront (CPU): Noll's index mapping and the Zernike polynomials against closed forms, the
normal-equation solve and its rank, the pupil basis, and argument checks that come before any GPU call."""
import math

import numpy as np
import pytest

from pyrayt_amd.frame import (DeviceFrame, noll_index, pupil_axes, solve_normal_equations, zernike_basis)

NOLL = {1: (0, 0), 2: (1, 1), 3: (1, -1), 4: (2, 0), 5: (2, -2), 6: (2, 2), 7: (3, -1), 8: (3, 1), 9: (3, -3),
        10: (3, 3), 11: (4, 0), 12: (4, 2), 13: (4, -2), 14: (4, 4), 15: (4, -4), 16: (5, 1), 17: (5, -1),
        18: (5, 3), 19: (5, -3), 20: (5, 5), 21: (5, -5), 22: (6, 0), 35: (7, -7), 36: (7, 7), 37: (8, 0)}


def test_noll_index_to_n_m():
    for j, nm in NOLL.items():
        assert noll_index(j) == nm, j
    with pytest.raises(ValueError):
        noll_index(0)


def test_zernike_polynomials_against_closed_forms():
    rng = np.random.default_rng(1)
    rho, theta = np.sqrt(rng.random(500)), rng.random(500) * 2 * np.pi
    z = zernike_basis(15, rho, theta)
    closed = {
        1: np.ones_like(rho), 2: 2 * rho * np.cos(theta), 3: 2 * rho * np.sin(theta),
        4: math.sqrt(3) * (2 * rho ** 2 - 1), 5: math.sqrt(6) * rho ** 2 * np.sin(2 * theta),
        6: math.sqrt(6) * rho ** 2 * np.cos(2 * theta), 7: math.sqrt(8) * (3 * rho ** 3 - 2 * rho) * np.sin(theta),
        8: math.sqrt(8) * (3 * rho ** 3 - 2 * rho) * np.cos(theta), 9: math.sqrt(8) * rho ** 3 * np.sin(3 * theta),
        10: math.sqrt(8) * rho ** 3 * np.cos(3 * theta), 11: math.sqrt(5) * (6 * rho ** 4 - 6 * rho ** 2 + 1),
        12: math.sqrt(10) * (4 * rho ** 4 - 3 * rho ** 2) * np.cos(2 * theta),
        13: math.sqrt(10) * (4 * rho ** 4 - 3 * rho ** 2) * np.sin(2 * theta),
        14: math.sqrt(10) * rho ** 4 * np.cos(4 * theta), 15: math.sqrt(10) * rho ** 4 * np.sin(4 * theta),
    }
    for j, want in closed.items():
        np.testing.assert_allclose(z[j - 1], want, rtol=0, atol=1e-13)


def test_zernike_basis_is_orthonormal_on_the_unit_disk():
    n = 400
    r = (np.arange(n) + 0.5) / n
    t = (np.arange(2 * n) + 0.5) / (2 * n) * 2 * np.pi
    rr, tt = np.meshgrid(r, t)
    z = zernike_basis(36, rr.ravel(), tt.ravel())
    w = (rr.ravel() / n) * (2 * np.pi / (2 * n)) / np.pi
    gram = (z * w) @ z.T
    np.testing.assert_allclose(gram, np.eye(36), atol=1e-3)  # (midpoint rule)


def sums_of(z, v, w):
    terms = z.shape[1]
    zz = (z * w[:, None]).T @ z
    return np.concatenate([zz[np.triu_indices(terms)], (z * w[:, None]).T @ v, [w.sum(), (w * v).sum(),
                                                                             (w * v * v).sum()]])


def test_solve_normal_equations_and_rank():
    rng = np.random.default_rng(2)
    rho, theta = np.sqrt(rng.random(3000)), rng.random(3000) * 2 * np.pi
    z = zernike_basis(15, rho, theta).T
    coef = rng.normal(size=15)
    v = z @ coef
    got, rank = solve_normal_equations(sums_of(z, v, np.ones(len(v)))[None], 15)
    assert rank[0] == 15
    np.testing.assert_allclose(got[0], coef, atol=1e-9)
    # a single ring: piston and defocus (and the other radial terms) are one function of theta
    ring = zernike_basis(15, np.full(400, 0.7), np.linspace(0, 2 * np.pi, 400, endpoint=False)).T
    _, rank = solve_normal_equations(sums_of(ring, ring @ coef, np.ones(400))[None], 15)
    assert rank[0] < 15
    # a group without rows
    got, rank = solve_normal_equations(np.zeros((1, 15 * 16 // 2 + 15 + 3)), 15)
    assert rank[0] == 0 and np.all(np.isnan(got[0]))


def test_pupil_axes():
    np.testing.assert_array_equal(pupil_axes(), [1, 0, 0, 0, 1, 0, 0, 0, 1])
    axes = pupil_axes(axis=(0, 0, 2)).reshape(3, 3)
    np.testing.assert_allclose(axes @ axes.T, np.eye(3), atol=1e-15)
    np.testing.assert_allclose(axes[0], [0, 0, 1])
    with pytest.raises(ValueError, match="axis"):
        pupil_axes(axis=(0, 0, 0))
    with pytest.raises(ValueError, match="basis"):
        pupil_axes(basis=((0, 1, 0), (0, 1, 0)))


def host_frame():
    rows = np.zeros((15, 6))
    rows[0] = [0, 0, 0, 1, 1, 1]
    rows[4] = [0, 1, 2, 0, 1, 2]
    return DeviceFrame(rows, [3, 3])


def test_wavefront_arguments_are_checked_before_the_gpu():
    frame = host_frame()
    with pytest.raises(ValueError, match="zernike"):
        frame.wavefront(1, zernike=37)
    with pytest.raises(ValueError, match="zernike"):
        frame.wavefront(1, zernike=0)
    with pytest.raises(NotImplementedError):
        frame.wavefront(1, group=object())
    with pytest.raises(ValueError, match="weights"):
        frame.wavefront(1, weights="brightness")
    with pytest.raises(ValueError, match="pupil_radius"):
        frame.wavefront(1, pupil_radius=-1)
    with pytest.raises(ValueError, match="reference"):
        frame.wavefront(1, reference="chief ray")
    with pytest.raises(ValueError, match="where"):
        frame.where(generation=1).wavefront(1)
    with pytest.raises(ValueError, match="select"):
        frame.select(np.array([True] * 6)).optical_path()
    with pytest.raises(ValueError, match="generation"):
        frame.generation(1).optical_path()
    with pytest.raises(ValueError, match="rows_per_generation"):
        DeviceFrame(frame.rows).optical_path()
    recorded = host_frame()
    recorded.origin = "record_only"
    with pytest.raises(ValueError, match="record_only"):
        recorded.wavefront(1)


def test_abi_entries_are_declared():
    from pyrayt_amd import engine

    for name in ("prt_frame_optical_path", "prt_frame_wavefront_workspace_bytes", "prt_frame_wavefront"):
        assert name in engine.EXPORTED_SYMBOLS
    assert engine.PRT_VERSION == 240

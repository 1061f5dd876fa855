#!/usr/bin/env python3
"""The polarised diffraction PSF behind a metal fold mirror (DeviceFrame.psf(fresnel=...)).  A singlet
images a point source at unit magnification; an aluminium mirror at 45 degrees folds the converging beam onto a
detector.  The mirror reflects s and p with different amplitudes and phases, and the angle of incidence changes across
the beam, so what arrives is no longer one polarisation state with one phase: the scalar PSF of ``Fresnel.apply()``
sees the losses as apodisation and nothing else, the vector PSF sums the fields themselves.  For linear and circular
input this prints

  * ``strehl``: the image at the focus over the perfect, lossless wave with parallel fields (comparable across rows);
  * ``strehl_apodized``: over the same amplitudes with phases and field directions aligned (the strict ratio);
  * the scalar ``psf()`` of ``Fresnel.apply()``, which is normalised like ``strehl_apodized``;
  * the throughput, and the Stokes parameters of the image's brightest pixel over its S0.

    python examples/polarised_psf.py [rays] [cone angle in degrees]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyrayt_amd as pyrayt  # noqa: E402
from pyrayt_amd.materials import Coating  # noqa: E402

ALUMINIUM = 0.96 + 6.69j  # (n + ik near 0.55 um)


def build(rays, cone_angle):
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    source = pyrayt.components.ConeOfRays(cone_angle=cone_angle).move_x(-4)           # at 2 f: the image lies near +4
    mirror = pyrayt.components.plane_mirror(0.2, aperture=(2.0, 2.0)).rotate_z(45).move_x(2)  # folds +x into -y
    detector = pyrayt.components.baffle((1, 1)).rotate_z(90).move(2, -2, 0)
    return pyrayt.RayTracer(source, [lens, mirror, detector], rays_per_source=rays), lens, mirror, detector


def best_focus(frame, detector):
    """The point closest to the lines of the rays that reach the detector: sum (I - d d^T) (P - Q) = 0."""
    rows = frame.where(surface=detector.get_id())
    q = torch.stack([rows[name] for name in ("x1", "y1", "z1")], dim=1)
    d = torch.stack([rows[name] for name in ("x_tilt", "y_tilt", "z_tilt")], dim=1)
    d = d / d.norm(dim=1, keepdim=True)
    across = torch.eye(3, dtype=q.dtype, device=q.device)[None] - d[:, :, None] * d[:, None, :]
    return torch.linalg.solve(across.sum(dim=0), (across @ q[:, :, None]).sum(dim=0)[:, 0]).cpu().numpy()


def main():
    rays = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
    cone_angle = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
    tracer, lens, mirror, detector = build(rays, cone_angle)
    frame = tracer.trace_device()
    wavelength = float(frame["wavelength"][0])
    focus = best_focus(frame, detector)
    options = dict(world_unit_um=1000.0, pixels=64, reference=focus, axis=(0.0, -1.0, 0.0))
    coatings = {lens: Coating.quarter_wave(1.38, wavelength), mirror: Coating((), substrate=ALUMINIUM)}
    print(f"{rays} rays, a {cone_angle:g} degree cone, {wavelength:g} um; focus at ({focus[0]:.4f}, {focus[1]:.4f}, {focus[2]:.4f})")
    bare = frame.psf(detector, **options)
    print(f"{'no losses (scalar psf)':<26} strehl {bare.strehl[0]:.5f}")
    print(f"{'input':<26} {'strehl':>8} {'apodized':>9} {'scalar':>8} {'through':>8}   S1/S0   S2/S0   S3/S0  axial/S0")
    inputs = (("linear y (p at the fold)", (0, 1, 0)), ("linear z (s at the fold)", (0, 0, 1)), ("linear 45 degrees", (0, 1, 1)),
              ("circular", (0, 1, 1j)), ("unpolarised", None))
    for label, polarization in inputs:
        fresnel = frame.fresnel(polarization=polarization, coatings=coatings, fields=True)
        vector = frame.psf(detector, fresnel=fresnel, **options)
        scalar = fresnel.apply().psf(detector, **options)
        i, j = np.unravel_index(int(np.argmax(vector.image[0])), vector.image[0].shape)
        s0 = vector.stokes[0, 0, i, j]
        ratios = "  ".join(f"{vector.stokes[0, k, i, j] / s0:+.3f}" for k in (1, 2, 3))
        print(f"{label:<26} {vector.strehl[0]:8.5f} {vector.strehl_apodized[0]:9.5f} {scalar.strehl[0]:8.5f} "
              f"{vector.throughput[0]:8.5f}  {ratios}  {vector.axial[0, i, j] / s0:.2e}")
    print(f"{fresnel.n_coated} interfaces at coated surfaces, {fresnel.n_invalid} invalid rays")


if __name__ == "__main__":
    main()

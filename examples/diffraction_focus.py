#!/usr/bin/env python3
"""Where is a singlet's diffraction focus?  With spherical aberration the plane of the smallest RMS spot, the plane of
the largest Strehl ratio and the paraxial focus are three different planes.  One trace gives the first two: the
closed-form RMS-spot focus of the ray aberrations (DeviceFrame.ray_aberrations) and the through-focus diffraction PSF
(DeviceFrame.psf(focus=...)), a Huygens sum evaluated on 41 planes from the one wavefront, with no
re-trace.  It prints both shifts from the detector along the axis, and the Strehl ratio at each.

    python examples/diffraction_focus.py [rays] [beam diameter]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pyrayt_amd as pyrayt  # noqa: E402

RINGS = 16


def build(rays, diameter, detector_x=2.0):
    """A collimated beam of ``diameter`` as 16 rings of equal area (one group), a biconvex singlet, a detector."""
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    rings = [pyrayt.components.CircleOfRays(diameter=diameter * np.sqrt((k + 0.5) / RINGS)).move_x(-1) for k in range(RINGS)]
    detector = pyrayt.components.baffle((1, 1)).move_x(detector_x)
    return pyrayt.RayTracer(rings, [lens, detector], rays_per_source=max(1, rays // RINGS)), detector


def main(rays=32_000, diameter=0.7, verbose=True):
    tracer, detector = build(rays, diameter)
    frame = tracer.trace_device()
    spot = float(frame.ray_aberrations(detector).best_focus()[0])
    first = frame.psf(detector, world_unit_um=1000.0, pixels=8)
    depth = 2 * first.wavelengths[0] * 1e-3 * first.f_number[0] ** 2  # 2 lambda F^2
    # 41 planes from the detector past the RMS-spot focus, then the two planes themselves
    span = abs(spot) + 4 * depth
    scan = frame.psf(detector, world_unit_um=1000.0, pixels=8, focus=np.linspace(-span, span, 41))
    diffraction = float(scan.best_focus()[0])
    at = frame.psf(detector, world_unit_um=1000.0, pixels=8, focus=[diffraction, spot, 0.0])
    if verbose:
        print(f"{rays} rays, a beam of {diameter:g}, {first.wavelengths[0]:g} um, F/{first.f_number[0]:.1f}: "
              f"depth of focus 2 lambda F^2 = {depth:.4f}")
        print(f"{'plane':<28} {'shift along the axis':>21} {'Strehl':>8}")
        for label, shift, strehl in (("diffraction focus (psf scan)", diffraction, at.strehl[0, 0]),
                                     ("RMS-spot focus (aberrations)", spot, at.strehl[0, 1]),
                                     ("the detector", 0.0, at.strehl[0, 2])):
            print(f"{label:<28} {shift:>+21.5f} {strehl:>8.4f}")
        print(f"the two foci lie {abs(diffraction - spot) / depth:.2f} depths of focus apart")
    return dict(diffraction=diffraction, spot=spot, depth=depth, strehl=at.strehl[0].tolist())


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32_000, float(sys.argv[2]) if len(sys.argv) > 2 else 0.7)

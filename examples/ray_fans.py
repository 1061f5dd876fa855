#!/usr/bin/env python3
"""Ray-aberration curves of a singlet from one trace: the longitudinal curve of the reference's
examples/lens_design.ipynb (cells 12-13: focus against the height at which a ray entered), the tangential and sagittal
fans every lens-design program draws beside the spot diagram, and the best focus in closed form -- past the last
surface a ray is a straight line, so the plane of the smallest RMS spot follows from the rays' positions and slopes
at any one plane (RayTracer.trace_ray_aberrations).

    python examples/ray_fans.py [rays]

The last step finds the same plane the way examples/best_focus.py does, by moving the detector and tracing again in a
golden-section search, and prints the two side by side."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402


def build(rays):
    """The notebook's singlet, lit by a collimated fan in the xy plane and one in the xz plane."""
    lens = pyrayt.components.thick_lens(40, -200, 5, aperture=25.4, material=pyrayt.materials.glass["BK7"])
    tangential = pyrayt.components.LineOfRays(spacing=16, wavelength=0.55).move_x(-50)
    sagittal = pyrayt.components.LineOfRays(spacing=16, wavelength=0.55).rotate_x(90).move_x(-50)
    detector = pyrayt.components.baffle((25.4, 25.4)).move_x(60)
    tracer = pyrayt.RayTracer([tangential, sagittal], [lens, detector], rays_per_source=rays // 2)
    return tracer, detector


def spot_radius(tracer, detector, x):
    detector.move_x(x - detector.get_position()[0])
    return float(tracer.trace_stats(surface=detector).values("last")["rms_radius"][0])


def golden_section(tracer, detector, a, b, tol=1e-5):
    g = (np.sqrt(5.0) - 1.0) / 2.0
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = spot_radius(tracer, detector, c), spot_radius(tracer, detector, d)
    traces = 2
    while b - a > tol:
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = spot_radius(tracer, detector, c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = spot_radius(tracer, detector, d)
        traces += 1
    return 0.5 * (a + b), traces


def main(rays=200_000, verbose=True):
    tracer, detector = build(rays)
    x_detector = detector.get_position()[0]
    got = tracer.trace_ray_aberrations(detector, zones=16, rays_per_source=True)   # group 0: the xy fan, 1: the xz fan
    best, radius = float(got.best_focus()[0]), float(got.rms_radius(got.best_focus()[0])[0])
    curve = got.longitudinal_curve()
    if verbose:
        print(f"{got.n_rays.sum()} rays on the detector at x = {x_detector:g}, {got.n_missed.sum()} left out")
        # (the notebook's axis crossing is taken in the xy plane: it is the xy fan that has one)
        print("longitudinal aberration (the notebook's cell 13): entry height, mean axis crossing, spread, rays")
        for h, mean, std, count in zip(curve["radius"][0], curve["mean"][0], curve["std"][0], curve["count"][0]):
            print(f"  {h:7.3f}  {mean:10.5f}  {std:9.2e}  {count}")
        for group, (name, azimuth) in enumerate((("tangential", 0.0), ("sagittal", 90.0))):
            t, along, _ = got.fan(azimuth, samples=9, focus=best)
            print(f"{name} fan at best focus (pupil position, transverse aberration):")
            print("  " + "  ".join(f"{p:+.2f}:{e:+.2e}" for p, e in zip(t, along[group])))
        print(f"best focus in closed form: x = {x_detector + best:.5f} (RMS spot radius {radius:.3e}), from one trace")
    searched, traces = golden_section(tracer, detector, x_detector + best - 2.0, x_detector + best + 2.0)
    if verbose:
        print(f"best focus by golden-section search: x = {searched:.5f}, from {traces} traces")
    return x_detector + best, searched


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)

#!/usr/bin/env python3
"""Fresnel losses of a biconvex lens (DeviceFrame.fresnel / RayTracer.trace_fresnel).  The engine's
intensity column is lossless: a ray leaves its source at 100 and arrives at 100 however much glass it crossed.  This
takes the biconvex lens of the README, an on-axis and an off-axis source, and reports per source

  * the throughput: the energy at the detector over the energy launched (Fresnel.transmission);
  * the radius that encloses 80 % of the energy at the detector (enclosed_energy on the frame Fresnel.apply() returns);
  * the relative illumination: the off-axis source's throughput over the on-axis source's;

without losses, with the losses of the uncoated surfaces, and with the lens declared lossless (ideally coated).

    python examples/fresnel_losses.py [rays per source] [field angle in degrees]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402


def build(rays, field_angle):
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    on_axis = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-2)
    off_axis = pyrayt.components.ConeOfRays(cone_angle=6).rotate_z(field_angle).move_x(-2)
    detector = pyrayt.components.baffle((2, 2)).move_x(1)
    return pyrayt.RayTracer([on_axis, off_axis], [lens, detector], rays_per_source=rays), lens, detector


def report(label, frame, throughput, detector, rays):
    energy = frame.enclosed_energy(detector, fractions=(0.8,), rays_per_source=rays, n_groups=2)
    print(f"{label:<22} throughput {throughput[0]:.4f} / {throughput[1]:.4f}   "
          f"EE80 radius {energy.radius[0, 0, 0]:.5f} / {energy.radius[1, 0, 0]:.5f}   "
          f"relative illumination {throughput[1] / throughput[0]:.4f}")


def main():
    rays = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    field_angle = float(sys.argv[2]) if len(sys.argv) > 2 else 5.0
    tracer, lens, detector = build(rays, field_angle)
    frame = tracer.trace_device()
    print(f"on-axis / {field_angle:g} degrees off-axis, {rays} rays each")

    coated = frame.fresnel(lossless=lens)
    report("lossless frame", frame, coated.transmission(detector, rays_per_source=rays), detector, rays)
    losses = frame.fresnel()
    report("uncoated (Fresnel)", losses.apply(), losses.transmission(detector, rays_per_source=rays), detector, rays)
    report("lens declared lossless", coated.apply(), coated.transmission(detector, rays_per_source=rays), detector, rays)
    print(f"interfaces: {losses.n_reflections} reflections (ideal unless coated), {losses.n_undeviated} undeviated, "
          f"{losses.n_invalid} invalid rays; {coated.n_lossless} at coated surfaces")
    layer = pyrayt.materials.Coating.quarter_wave(1.38, float(frame["wavelength"][0]))  # (MgF2, a quarter wave thick)
    quarter = frame.fresnel(coatings={lens: layer})
    report("quarter-wave MgF2", quarter.apply(), quarter.transmission(detector, rays_per_source=rays), detector, rays)
    polarised = frame.fresnel(polarization=(0.0, 1.0, 0.0)).transmission(detector, rays_per_source=rays)
    print(f"input polarised along y: throughput {polarised[0]:.4f} / {polarised[1]:.4f}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Diffraction PSF of the frame on the device (DeviceFrame.psf, RayTracer.trace_psf), timed with device events after
warm-up, on BASELINE config 2 (3 generations; the detector holds one row per ray).

  wavefront     DeviceFrame.wavefront(detector, weights="intensity"): what psf() runs first
  psf_<n>       DeviceFrame.psf(detector, pixels=n): the wavefront passes, the PSF passes, the image brought back;
                with the rate in ray-pixel terms per second (rays summed x pixels / time), of the whole call and of
                the call less the wavefront
  loop          trace_psf(detector) end to end, against trace_device() alone
  numpy         the definition restated in numpy on the host (one core), on a sample of the rays and pixels: its rate
                in terms per second, for comparison

Prints one JSON line per figure.  usage: tools/psf_bench.py [--rays N] [--steps K] [--pixels 64 128]
(run under rocprofv3 --kernel-trace --stats for per-kernel times)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402


def device_ms(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def wall_ms(fn, steps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def numpy_rate(psf, rays=20_000, pixels=256):
    """terms per second of the numpy restatement of the Huygens sum (one wavelength, complex128, one core)"""
    wave = psf.wavefront
    opd = wave.opd[:rays].cpu().numpy()
    p1 = wave.pupil[:rays, 0].cpu().numpy() * wave.pupil_radius[0]
    radius, lw = wave.radius[0], psf.wavelengths[0] / psf.world_unit_um
    u = np.linspace(-1, 1, pixels) * psf.pixel_size[0] * 8
    t = time.perf_counter()
    for k in range(pixels):
        d = np.sqrt(radius ** 2 + u[k] ** 2 - 2 * u[k] * p1)
        np.exp(2j * np.pi * (opd + d - radius) / lw).sum()
    return len(opd) * pixels / (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--pixels", type=int, nargs="+", default=[64, 128])
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame)}
    wave_ms = device_ms(lambda: frame.wavefront(det, weights="intensity"), args.steps)
    print(json.dumps({**common, "what": "wavefront", "ms": wave_ms}), flush=True)
    psf = None
    for n in args.pixels:
        psf = frame.psf(det, world_unit_um=1000.0, pixels=n)
        ms = device_ms(lambda: frame.psf(det, world_unit_um=1000.0, pixels=n), args.steps)
        terms = float(psf.n_rays.sum()) * n * n
        print(json.dumps({**common, "what": f"psf_{n}", "ms": ms, "terms": terms,
                          "terms_per_s_whole_call": terms / (ms * 1e-3),
                          "terms_per_s_without_wavefront": terms / ((ms - wave_ms) * 1e-3)}), flush=True)
    trace_only = wall_ms(tracer.trace_device, args.steps)
    loop = wall_ms(lambda: tracer.trace_psf(det, world_unit_um=1000.0), args.steps)
    print(json.dumps({**common, "what": "loop", "pixels": 128, "trace_device_ms": trace_only, "trace_psf_ms": loop}),
          flush=True)
    print(json.dumps({**common, "what": "numpy", "terms_per_s": numpy_rate(psf)}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Fresnel transmittance of the frame on the device (DeviceFrame.fresnel), timed with device events after warm-up, on
BASELINE config 2 at --rays rays (3 generations, two refractions a ray):

  fresnel         DeviceFrame.fresnel() end to end (the launches and the read-back of the status word and counters)
  fresnel_fields  the same with the per-row fields written out
  apply           Fresnel.apply(): the copy of the rows and the multiply
  optical_path    the yardstick: DeviceFrame.optical_path(), the other per-generation pass over a dense per-id state
  host            the host route: copy eight columns, pandas join by id, numpy Fresnel (the scalar mean of T_s and T_p
                  per interface, which is less than the device computes) (wall time, one core)

Prints one JSON line per figure.  usage: tools/fresnel_bench.py [--rays N] [--steps K] [--no-host]
(run under rocprofv3 --kernel-trace --stats for per-kernel times: k_fresnel_step against k_frame_optical_path)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from mtf_bench import device_ms  # noqa: E402
from pyrayt_amd.frame import _FRESNEL_COLUMNS  # noqa: E402


def host_fresnel(frame):
    """The host route: eight columns brought over, each row joined with the same ray's row of the generation before,
    the unpolarised Fresnel transmittance per interface and its running product per ray."""
    table = pd.DataFrame({name: frame[name].cpu().numpy() for name in _FRESNEL_COLUMNS})
    before = table.assign(generation=table["generation"] + 1)
    joined = table.merge(before, on=["id", "generation"], how="left", suffixes=("", "_i"))
    ut = joined[["x_tilt", "y_tilt", "z_tilt"]].to_numpy()
    ui = joined[["x_tilt_i", "y_tilt_i", "z_tilt_i"]].to_numpy()
    ni, nt = joined["index_i"].to_numpy(), joined["index"].to_numpy()
    with np.errstate(all="ignore"):
        normal = ni[:, None] * ui - nt[:, None] * ut
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        ci, ct = np.abs(np.sum(ui * normal, axis=1)), np.abs(np.sum(ut * normal, axis=1))
        a, b, c, d = ni * ci, nt * ct, nt * ci, ni * ct
        step = 0.5 * (4 * a * b / (a + b) ** 2 + 4 * a * b / (c + d) ** 2)
    joined["step"] = np.where(np.isfinite(step) & (ni != nt), step, 1.0)
    joined = joined.sort_values(["id", "generation"], kind="stable")
    return joined.groupby("id")["step"].cumprod()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation)}
    got = frame.fresnel()
    through = float(got.transmission(det)[0])
    ms = device_ms(lambda: frame.fresnel(), args.steps)
    print(json.dumps({**common, "what": "fresnel", "ms": ms, "transmission": through, "n_invalid": got.n_invalid}), flush=True)
    ms = device_ms(lambda: frame.fresnel(fields=True), args.steps)
    print(json.dumps({**common, "what": "fresnel_fields", "ms": ms}), flush=True)
    ms = device_ms(lambda: got.apply(), args.steps)
    print(json.dumps({**common, "what": "apply", "ms": ms}), flush=True)
    ms = device_ms(lambda: frame.optical_path(), args.steps)
    print(json.dumps({**common, "what": "optical_path", "ms": ms}), flush=True)
    if not args.no_host:
        t = time.perf_counter()
        product = host_fresnel(frame)
        print(json.dumps({**common, "what": "host", "copy_join_fresnel_ms": (time.perf_counter() - t) * 1e3,
                          "least": float(product.min())}), flush=True)


if __name__ == "__main__":
    main()

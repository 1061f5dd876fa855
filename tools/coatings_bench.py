#!/usr/bin/env python3
"""The coated Fresnel step on the device (DeviceFrame.fresnel(coatings=...)), timed with device events after warm-up, on
config 2's lens at --rays rays, against fresnel() of the same frame and against the host route:

  fresnel            DeviceFrame.fresnel() end to end: k_fresnel_step, the yardstick
  coated_none        fresnel(coatings={}): the coated kernel with nothing coated
  coated_quarter     one quarter-wave layer of index 1.38 on the lens
  coated_16          16 layers on the lens
  host               the host route: copy nine columns, pandas join by id, the numpy restatement of
                     tests/coating_reference.py per interface (timed on --host-rays rays' rows and scaled by rows)

Prints one JSON line per figure.  usage: tools/coatings_bench.py [--rays N] [--steps K] [--no-host]
(run under rocprofv3 --kernel-trace --stats, in a run of its own, for per-kernel times: k_coated_fresnel_step against
k_fresnel_step)"""
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

import coating_reference as cr  # noqa: E402
import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from mtf_bench import device_ms  # noqa: E402
from pyrayt_amd.frame import _FRESNEL_COATED_COLUMNS  # noqa: E402
from pyrayt_amd.materials import Coating  # noqa: E402


def host_route(frame, coatings, rays):
    """Nine columns brought over, the rows of the first `rays` ids joined with pandas (what orders them by generation and
    id), the numpy restatement on them: (seconds for the copy, seconds for join + restatement, rows handled)."""
    t = time.perf_counter()
    table = pd.DataFrame({name: frame[name].cpu().numpy() for name in _FRESNEL_COATED_COLUMNS})
    copied = time.perf_counter() - t
    t = time.perf_counter()
    part = table[table["id"] < table["id"].min() + rays]
    before = part.assign(generation=part["generation"] + 1)
    joined = part.merge(before[["id", "generation"]], on=["id", "generation"], how="left")
    rows = np.zeros((len(joined), 15))
    for name in _FRESNEL_COATED_COLUMNS:
        rows[:, cr.IX[name]] = joined[name].to_numpy()
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    cr.fresnel(rows, coatings=coatings)
    return copied, time.perf_counter() - t, len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-rays", type=int, default=2000)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    wavelength = float(frame["wavelength"][0])
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation)}
    quarter = Coating.quarter_wave(1.38, wavelength)
    stack = cr.random_stack(5, 16, lam=wavelength)
    sixteen = Coating(stack.layers)
    cases = (("fresnel", None), ("coated_none", {}), ("coated_quarter", {lens: quarter}), ("coated_16", {lens: sixteen}))
    for what, coatings in cases:
        got = frame.fresnel(coatings=coatings)
        through = float(got.transmission(det)[0])
        ms = device_ms(lambda: frame.fresnel(coatings=coatings), args.steps)
        print(json.dumps({**common, "what": what, "ms": ms, "transmission": through, "n_invalid": got.n_invalid,
                          "n_coated": got.n_coated}), flush=True)
    ms = device_ms(lambda: frame.fresnel(coatings={lens: quarter}, fields=True), args.steps)
    print(json.dumps({**common, "what": "coated_quarter_fields", "ms": ms}), flush=True)
    if not args.no_host:
        ids = {sid: quarter for sid, _ in lens.surface_ids}
        copied, worked, rows = host_route(frame, ids, args.host_rays)
        print(json.dumps({**common, "what": "host", "copy_ms": copied * 1e3, "join_reference_ms_measured": worked * 1e3,
                          "rows_measured": rows,
                          "copy_join_reference_ms_scaled": copied * 1e3 + worked * 1e3 * len(frame) / max(rows, 1)}), flush=True)


if __name__ == "__main__":
    main()

"""What the four entry points and their size functions answer to bad arguments, on a machine without a GPU (every check
comes before a device is touched): python profiles/sensitivity_core/sens_refusals.py LIB.so > out.jsonl.  One line per (mutation, form)."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import launch_scenes  # noqa: E402
from pyrayt_amd import engine  # noqa: E402
from pyrayt_amd.engine import _pointer as _sens_pointer  # noqa: E402
from pyrayt_amd.frame import _SENS_FORMS  # noqa: E402
from pyrayt_amd.scene import PRIM_DTYPE, SceneSnapshot  # noqa: E402

engine.LIB_PATH = os.path.abspath(sys.argv[1])
lib = engine.library()
case = launch_scenes.build("cone", 16)
snap = SceneSnapshot(case.parts)
PRIMS = np.sort(np.asarray(snap.prims, dtype=PRIM_DTYPE), order="surface_id")
MATS = np.ascontiguousarray(snap.materials)
first_id = int(PRIMS["surface_id"][0])
K = 2
f8 = lambda *shape: np.zeros(shape, dtype=np.float64)  # noqa: E731


def base():
    return dict(device=0, rows=f8(15, 4), ld=4, counts=np.array([2, 2], dtype=np.int64), n_generations=2, id0=0.0, n_ids=2,
                prims=PRIMS.copy(), n_prims=len(PRIMS), twists=f8(K, 9), parameter_ids=np.array([first_id, first_id], dtype=np.int64),
                parameter_first=np.array([0, 0, 1], dtype=np.int32), linear=f8(K, 9), index_rates=f8(K),
                index_ids=np.array([first_id, first_id], dtype=np.int64), index_first=np.array([0, 0, 1], dtype=np.int32), K=K,
                row_slot=np.array([-1, -1, 0, 1], dtype=np.int64), selected=np.array([2, 3], dtype=np.int64), n_selected=2,
                group_first=np.array([0, 2], dtype=np.int64), n_groups=1, weight_column=-1, pivots=f8(3), opl=f8(4),
                groups=np.array([[0, 0, 0, 1, 0, 1]], dtype=np.float64), axes=np.eye(3).reshape(-1).copy(), n_terms=4,
                ranges=f8(K, 2), flags=np.zeros(K, dtype=np.int32), colour_rates=f8(K), materials=MATS.copy(),
                n_materials=len(MATS), jacobian=f8(K, 3, 2), sums=f8(1, 64), slopes=f8(K, 3, 2), dfield=f8(K, 2), dopd=f8(K, 2),
                dpupil=f8(K, 2, 2), opd=f8(2), pupil=f8(2, 2), opd_sums=f8(1, 256), record=np.zeros(4, dtype=np.int64),
                work=np.zeros(1 << 20, dtype=np.uint8), stream=None)


def changed(name, how):
    def apply(p):
        p[name] = how(p[name]) if callable(how) else how
    return apply


def put(index, value):
    def how(array):
        array = array.copy()
        array.reshape(-1)[index] = value
        return array
    return how


def prim_field(field, index, value):
    def how(prims):
        prims = prims.copy()
        prims[field][index] = value
        return prims
    return how


ONE = {f"{name}=NULL": changed(name, None) for name in (
    "record", "work", "sums", "prims", "twists", "parameter_first", "group_first", "pivots", "rows", "row_slot", "selected",
    "jacobian", "linear", "index_rates", "index_first", "index_ids", "parameter_ids", "groups", "axes", "opd_sums", "dfield",
    "dopd", "dpupil", "opd", "pupil", "opl", "ranges", "flags", "colour_rates", "materials", "slopes", "counts")}
ONE.update({
    "valid": lambda p: None,
    "n_selected=-1": changed("n_selected", -1), "n_selected=5": changed("n_selected", 5), "n_terms=0": changed("n_terms", 0),
    "n_terms=37": changed("n_terms", 37), "axes nan": changed("axes", put(4, np.nan)), "ld=1": changed("ld", 1),
    "counts negative": changed("counts", put(1, -2)), "n_generations=0": changed("n_generations", 0),
    "id0=0.5": changed("id0", 0.5), "id0 nan": changed("id0", float("nan")), "n_ids=0": changed("n_ids", 0),
    "K=0": changed("K", 0), "K=17": changed("K", 17), "n_groups=0": changed("n_groups", 0),
    "n_groups=70000": changed("n_groups", 70000), "weight_column=-2": changed("weight_column", -2),
    "weight_column=15": changed("weight_column", 15), "n_prims=0": changed("n_prims", 0),
    "group_first from 1": changed("group_first", put(0, 1)), "group_first to 1": changed("group_first", put(1, 1)),
    "pivots nan": changed("pivots", put(1, np.nan)), "radius 0": changed("groups", put(5, 0.0)),
    "radius nan": changed("groups", put(5, np.nan)), "type 99": changed("prims", prim_field("type", 1, 99)),
    "normal_scale 0": changed("prims", prim_field("normal_scale", 1, 0)), "unsorted": changed("prims", lambda q: q[::-1].copy()),
    "minv inf": changed("prims", lambda q: prim_field("minv", 0, np.full_like(q["minv"][0], np.inf))(q)),
    "parameter_first from 1": changed("parameter_first", put(0, 1)),
    "parameter_first descends": changed("parameter_first", put(1, 2)),
    "parameter_first 70 ids": changed("parameter_first", np.array([0, 70, 70], dtype=np.int32)),
    "twists nan": changed("twists", put(3, np.nan)), "parameter id unknown": changed("parameter_ids", put(0, 123456789)),
    "index_first from 1": changed("index_first", put(0, 1)), "index_first 70 ids": changed("index_first", np.array([0, 70, 70], dtype=np.int32)),
    "linear nan": changed("linear", put(10, np.nan)), "index rate inf": changed("index_rates", put(1, np.inf)),
    "index id unknown": changed("index_ids", put(0, 123456789)), "flags 4": changed("flags", put(0, 4)),
    "flags -1": changed("flags", put(1, -1)), "range descends": changed("ranges", put(0, 3.0)),
    "range nan": changed("ranges", put(1, np.nan)), "colour rate nan": changed("colour_rates", put(0, np.nan)),
    "a launch parameter with surfaces": changed("flags", put(1, 1)), "colour": changed("flags", put(0, 2)),
    "n_materials=0": changed("n_materials", 0), "material -1": changed("prims", prim_field("material", 0, -1)),
    "material kind 99": changed("materials", lambda m: prim_field("kind", slice(None), 99)(m)),
    "device=99": changed("device", 99),
})
PAIRS = [("K=0", "n_groups=0"), ("pivots nan", "type 99"), ("twists nan", "parameter id unknown"), ("linear nan", "flags 4"),
         ("group_first from 1", "weight_column=15"), ("n_terms=37", "id0 nan"), ("axes nan", "K=17"),
         ("unsorted", "parameter_first from 1"), ("index rate inf", "index id unknown"), ("radius 0", "minv inf"),
         ("parameter id unknown", "index_first from 1"), ("index id unknown", "range descends"), ("flags 4", "n_materials=0"),
         ("colour", "material kind 99"), ("record=NULL", "K=17"), ("ranges=NULL", "index id unknown"),
         ("minv inf", "twists nan"), ("n_selected=5", "n_terms=37"), ("ld=1", "work=NULL"), ("n_ids=0", "axes nan"),
         ("weight_column=-2", "n_prims=0"), ("radius nan", "unsorted"), ("parameter_first 70 ids", "twists nan"),
         ("index_first 70 ids", "linear nan"), ("material -1", "colour rate nan")]

for name, mutations in itertools.chain(((n, [n]) for n in ONE), ((" + ".join(p), list(p)) for p in PAIRS)):
    for form, (_, entry, order) in _SENS_FORMS.items():
        pieces = base()
        for m in mutations:
            ONE[m](pieces)
        rc = getattr(lib, entry)(*(_sens_pointer(pieces[q]) for q in order + ("work", "stream")))
        text = lib.prt_last_error().decode("utf-8", "replace") if rc else ""
        print(json.dumps({"what": name, "form": form, "rc": rc, "text": text}))

sizes = list(itertools.product((0, 1, 600, 1 << 40), (0, 4, (1 << 20) + 1), (0, 1, 5, 16, 17), (0, 1, 2, 65535, 65536),
                               (-1, 0, 1, 256, 257, 300, 1 << 33, 1 << 40)))
for form, (extra, entry, _) in _SENS_FORMS.items():
    size = entry + "_workspace_bytes"
    for args in sizes:
        for n_terms in ((-1, 0, 1, 15, 36, 37) if extra else (None,)):
            more = () if n_terms is None else (n_terms,)
            print(json.dumps({"size": size, "args": list(args + more), "bytes": getattr(lib, size)(*args, *more)}))

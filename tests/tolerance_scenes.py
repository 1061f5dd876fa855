"""Perturbed systems for the tolerancing tests: a scene of tests/opd_scenes.py built afresh with SEVERAL of its parameters
applied at once (``parameters[k].apply(amount)``) and traced on the CPU by the C oracle.  The scene files themselves stay
as they are; an ``IndexChange`` has no ``apply`` (its builders put the index into the glass) and is left at zero here."""
from types import SimpleNamespace

import opd_scenes
from sensitivity_scenes import trace


def applicable(parameters):
    """The parameters a trial may move: those with an ``apply``."""
    return [k for k, p in enumerate(parameters) if hasattr(p, "apply")]


def build(name, n, amounts):
    """Scene ``name`` with n rays, every parameter k changed by ``amounts[k]`` (0.0: left alone), re-traced."""
    fresh = opd_scenes._BUILDERS[name](n, None)  # (new parts: nothing cached is touched)
    assert len(amounts) == len(fresh.parameters)
    for k, amount in enumerate(amounts):
        if amount != 0.0:
            assert hasattr(fresh.parameters[k], "apply"), f"parameter {k} of {name} cannot be applied to a built system"
            fresh.parameters[k].apply(float(amount))
    frame, counts = trace(fresh.parts, fresh.rays, fresh.limit)
    return SimpleNamespace(name=name, parts=fresh.parts, frame=frame, counts=counts, surface=fresh.surface,
                           parameters=fresh.parameters, rays_per_source=getattr(fresh, "rays_per_source", None))

"""``device_run``: ``prt_frame_energy_tolerance`` (include/prt.h) on per-group trials -- the library call under
``Sensitivity.energy_tolerance``, which hands it the same trials for every group; the name is also for those who hand
the entry point trials that differ by group."""
import numpy as np

from . import engine
from .frame import _ENERGY_SHAPES


def device_run(head, jacobian, slopes, centres, axes, shape, follow_centroid, radii, fractions, planes, trials, compensate):
    """The entry point on the selected rows ``head`` (``Sensitivity._selected_rows()``) and host ``trials`` (groups, M,
    K), which may differ by group.  ``shape``: a name of ``enclosed_energy``'s; ``radii``, ``fractions`` (either may be
    empty, not both) and ``planes``: float64 arrays.  Returns host arrays: count (groups, M, F, R) uint64, energy
    (groups, M, F, R), radius (groups, M, F, N), moments (groups, M, 8), focus_shift (groups, M) and record (groups, 8):
    ``mtf_tolerance``'s seven doubles, then the bit image of W."""
    import torch

    dev, n_groups = head.rows.device, head.n_groups
    trials = np.ascontiguousarray(trials, dtype=np.float64)
    M, K = trials.shape[1:]
    assert trials.shape[0] == n_groups and K == jacobian.shape[0], (trials.shape, n_groups, jacobian.shape)
    radii, fractions, planes = (np.ascontiguousarray(v, dtype=np.float64) for v in (radii, fractions, planes))
    F, R, N = len(planes), len(radii), len(fractions)
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    count = torch.empty((n_groups, M, F, R), dtype=torch.int64, device=dev)  # (uint64 on the device: below 2^62)
    energy, radius = empty(n_groups, M, F, R), empty(n_groups, M, F, N)
    moments, shift, record = empty(n_groups, M, 8), empty(n_groups, M), empty(n_groups, 8)
    # (radii or fractions that were not asked for are NULL, and so are the outputs that would hold them: they are empty)
    engine.call("prt_frame_energy_tolerance", *head, jacobian.contiguous(), slopes.contiguous(), K, centres, axes,
                _ENERGY_SHAPES[shape], 1 if follow_centroid else 0, radii if R else None, R, fractions if N else None, N,
                planes, F, torch.as_tensor(trials, device=dev), M, int(bool(compensate)), count, energy, radius, moments,
                shift, record, device=dev, size=(head.n_selected, n_groups, K, R, N, F, M))
    return (engine.host(count).view(np.uint64), engine.host(energy), engine.host(radius), engine.host(moments),
            engine.host(shift), engine.host(record))

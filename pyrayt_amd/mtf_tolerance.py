"""The device call of ``Sensitivity.mtf_tolerance`` (pyrayt_amd/frame.py): Monte Carlo tolerancing of the geometric MTF,
the entry point ``prt_frame_mtf_tolerance`` of include/prt.h through ``engine.call``.  The checks of the arguments and the
result object (``MTFToleranceRun``) are frame.py's; here are the device buffers, the call and the read-back."""
import numpy as np


def device_run(head, jacobian, slopes, centres, axes, frequencies, azimuths, planes, trials, compensate_focus):
    """``head``: the selected rows of the sensitivity call (``Sensitivity._selected_rows()``); ``jacobian``, ``slopes``:
    its device (K, 3, n_selected) tensors; ``centres``: a device (groups, 3) tensor or None for the centroids; ``axes``,
    ``frequencies``, ``azimuths``, ``planes``: host float64 arrays; ``trials``: a host (groups, M, K) float64 array,
    finite.  Returns host arrays: otf (groups, M, F, A, N) complex, moments (groups, M, 8), focus_shift (groups, M),
    record (groups, 7)."""
    import torch

    from . import engine

    dev, n_groups = head.rows.device, head.n_groups
    trials = np.ascontiguousarray(trials, dtype=np.float64)
    M, K = trials.shape[1:]
    assert trials.shape[0] == n_groups and K == jacobian.shape[0], (trials.shape, n_groups, jacobian.shape)
    shape = (len(planes), len(azimuths), len(frequencies))
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    otf, moments, shift, record = empty(n_groups, M, *shape, 2), empty(n_groups, M, 8), empty(n_groups, M), empty(n_groups, 7)
    engine.call("prt_frame_mtf_tolerance", *head, jacobian.contiguous(), slopes.contiguous(), K, centres, axes, frequencies,
                len(frequencies), azimuths, len(azimuths), planes, len(planes), torch.as_tensor(trials, device=dev), M,
                int(bool(compensate_focus)), otf, moments, shift, record, device=dev,
                size=(head.n_selected, n_groups, K, len(frequencies), len(azimuths), len(planes), M))
    return engine.host_complex(otf), engine.host(moments), engine.host(shift), engine.host(record)

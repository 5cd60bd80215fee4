"""Neighbourhood limits from the user's own clouds: calibrate_neighbors on the HIP library.

The reference's calibrate_neighbors (src/models/backbone_kpconv/kpconv.py:714-747) collates one sample at a time
with rows of hist_n = ceil(4/3 pi (deform_radius + 1)^3) columns, counts the neighbours of every conv row per
level, histograms the counts and returns, per level, the count below which `keep_ratio` of the neighbourhoods
fall.  Here no row is ever written: per level one cell table and one count-only walk of it
(ops.RadiusTable.count -> spr_radius_table_count) histogram the counts per cloud on the device, for `chunk`
samples at once, and the host keeps the reference's bookkeeping -- the per-sample accumulation, its early stop
and its two percentile lines -- as they stand.  Everything is integer-exact: the histograms, and so the limits,
are those of the reference's procedure over its CPU extensions.

One deliberate difference: the reference sizes its histogram by config.num_layers, which equals the number of
pyramid levels in none of the shipped YAML files (its `+=` of the per-level histograms would fail there).  Here
the histogram has one row per level of plan_pyramid(config).
"""
import logging
from typing import Sequence

import numpy as np
import torch

from . import ops

_logger = logging.getLogger(__name__)

ROW_WIDTH_MAX = 128     # the widest neighbour row the library's searches produce (include/spr.h)


def hist_width(config) -> int:
    """Upper bound of the neighbour count worth binning (kpconv.py:719)."""
    return int(np.ceil(4 / 3 * np.pi * (config.deform_radius + 1) ** 3))


def _add_sample(total: np.ndarray, sample: np.ndarray, samples_threshold) -> bool:
    """Adds one sample's [levels, hist_n] histogram to `total` in place; True when the reference's loop stops behind
    this sample (kpconv.py:738): EVERY level's total exceeds samples_threshold, strictly."""
    total += sample
    return bool(np.min(np.sum(total, axis=1)) > samples_threshold)


def stop_index(sample_hists: Sequence[np.ndarray], samples_threshold) -> int:
    """Number of samples the reference's loop uses (kpconv.py:723-739): it accumulates in dataset order and stops
    after the first sample at which every level's histogram total exceeds samples_threshold; all of them when that
    never happens.  sample_hists: per sample an integer [levels, hist_n] array."""
    total = np.zeros_like(np.asarray(sample_hists[0], np.int64)) if len(sample_hists) else None
    for i, h in enumerate(sample_hists):
        if _add_sample(total, np.asarray(h, np.int64), samples_threshold):
            return i + 1
    return len(sample_hists)


def limits_from_hists(hists: np.ndarray, keep_ratio: float = 0.8) -> np.ndarray:
    """The reference's two percentile lines (kpconv.py:741-743), in float64 numpy: per level the number of counts k
    whose cumulative share stays below keep_ratio."""
    hists = np.asarray(hists)
    hist_n = hists.shape[1]
    cumsum = np.cumsum(hists.T, axis=0)
    return np.sum(cumsum < (keep_ratio * cumsum[hist_n - 1, :]), axis=0)


def coverage(hists: np.ndarray, limits) -> np.ndarray:
    """[levels] float64: the share of the binned neighbourhoods of a level that a row of limits[level] columns keeps
    whole (count <= limit).  NaN for a level without a binned neighbourhood."""
    hists = np.asarray(hists, np.int64)
    out = np.full((len(limits),), np.nan)
    for l, lim in enumerate(limits):
        total = int(hists[l].sum())
        if total > 0:
            out[l] = float(hists[l, :max(int(lim) + 1, 0)].sum()) / total
    return out


def _cloud(x, device) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else torch.as_tensor(x)
    return t.to(device=device, dtype=torch.float32).reshape(-1, 3)


def _chunk_hists(clouds, levels, config, hist_n: int) -> np.ndarray:
    """int64 [levels, clouds, hist_n]: the conv-row count histogram of every cloud at every pyramid level, all clouds
    in one batched pass.  Per level: one cell table, one count-only self search where the level has a conv, one
    grid subsampling to the next level; one device->host copy of the histograms per level."""
    device = clouds[0].device
    points = torch.cat(clouds, dim=0).contiguous()
    cu = ops.lengths_to_cu([int(c.shape[0]) for c in clouds], device)
    out = np.zeros((len(levels), len(clouds), hist_n), np.int64)
    for l, lv in enumerate(levels):
        if lv.has_conv:
            table = ops.RadiusTable(points, cu, lv.conv_radius)   # the conv search's radius (kpconv.py:631-634)
            _, hist = table.count(table.supports, table.s_cu, hist_n, counts=False)
            out[l] = hist.cpu().numpy()
        if lv.down:
            dl = 2 * lv.radius / config.conv_radius          # kpconv.py:367
            points, sub_lens = ops.grid_subsample(points, cu, dl)
            cu = ops.lengths_to_cu(sub_lens, device)
    return out


def calibrate_neighbors(dataset, config, collate_fn=None, keep_ratio=0.8, samples_threshold=2000, chunk=8,
                        return_hists=False):
    """neighborhood_limits for `config` from the clouds of `dataset` (reference kpconv.py:714-747).

    dataset: a sequence whose items carry 'src_xyz' and 'tgt_xyz' ([n, 3]; numpy or torch, host or device), the
    reference's contract.  config: what plan_pyramid reads (first_subsampling_dl, conv_radius, architecture, the
    feature widths) and deform_radius; neighborhood_limits may be missing or None.  collate_fn exists for signature compatibility: the pyramid is
    built by this library, anything but None raises NotImplementedError.

    `chunk` samples (2 * chunk clouds) go through the pyramid in one batched pass; their histograms are added
    sample by sample in dataset order and the loop stops after the first sample at which every level's total
    exceeds samples_threshold, exactly like the reference -- samples behind that one add nothing even when their
    chunk was computed, so the result does not depend on `chunk`.

    The histogram has hist_n = ceil(4/3 pi (deform_radius + 1)^3) bins and one row per level of
    plan_pyramid(config) (the reference sizes it by config.num_layers, which does not match its own pyramid in
    any shipped YAML; see the module docstring).  A neighbourhood with hist_n or more points is not binned.

    Returns a numpy int array, one limit per level; with return_hists also the int64 [levels, hist_n] histogram
    and the number of samples used.  One log line per level reports the limit, the share of neighbourhoods it
    keeps whole and, where config.neighborhood_limits exists, the share the configured limit keeps.  A limit
    above 128 is returned as it is and reported as beyond the width of the library's neighbour rows."""
    from .kpconv import plan_pyramid
    if collate_fn is not None:
        raise NotImplementedError("calibrate_neighbors builds the pyramid itself; collate_fn must be None")
    if chunk < 1:
        raise ValueError("calibrate_neighbors: chunk must be >= 1")
    _, levels, _ = plan_pyramid(config)
    hist_n = hist_width(config)
    device = None
    hists = np.zeros((len(levels), hist_n), np.int64)
    used, done = 0, False
    for base in range(0, len(dataset), chunk):
        items = [dataset[i] for i in range(base, min(base + chunk, len(dataset)))]
        if device is None:      # clouds already on a device decide where the work runs; host inputs go to the current one
            first = items[0]['src_xyz']
            device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device(
                'cuda', torch.cuda.current_device())
        clouds = [_cloud(it[k], device) for it in items for k in ('src_xyz', 'tgt_xyz')]
        per_cloud = _chunk_hists(clouds, levels, config, hist_n)
        for s in range(len(items)):
            used += 1
            if _add_sample(hists, per_cloud[:, 2 * s] + per_cloud[:, 2 * s + 1], samples_threshold):
                done = True
                break
        if done:
            break
    limits = limits_from_hists(hists, keep_ratio)
    configured = getattr(config, 'neighborhood_limits', None)
    cov = coverage(hists, limits)
    # (the shipped 3DMatch list carries four entries for a pyramid of three levels: extra ones are not read)
    configured = None if configured is None else [int(v) for v in configured][:len(levels)]
    cov_cfg = None if configured is None else coverage(hists, configured)
    for l in range(len(levels)):
        line = f"calibrate_neighbors level {l}: limit {int(limits[l])} keeps {cov[l]:.3f} of {int(hists[l].sum())} neighbourhoods whole"
        if cov_cfg is not None and l < len(configured):
            line += f"; configured limit {int(configured[l])} keeps {cov_cfg[l]:.3f}"
        if limits[l] > ROW_WIDTH_MAX:
            line += f"; {int(limits[l])} is beyond the library's row width of {ROW_WIDTH_MAX}"
        _logger.info(line)
    if return_hists:
        return limits, hists, used
    return limits

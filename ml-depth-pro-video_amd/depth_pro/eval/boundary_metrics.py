"""The Depth Pro paper's boundary metric on the MI355X (drop-in for the reference's depth_pro/eval/boundary_metrics.py).

`SI_boundary_F1` and `SI_boundary_Recall` return what the reference returns for float32 inputs: the edge counts are
made on the device (csrc/dp_boundary.hip; the rules are in include/dp_mi355x.h) and equal the reference's exactly, and
the scores are made from them here with the reference's own float64 expressions and numpy's summation.

Differences, stated: depths must be float32 (the reference would work a float64 array through in float64; it is
refused here), and the results are counts, maps and scores -- nothing else is claimed.  There is no host fallback:
without the library or a ROCm device the calls raise.
"""

from __future__ import annotations

import ctypes
from typing import Tuple

import numpy as np
import torch

from .. import _lib
from .._lib import DP_BOUNDARY_DEPTH, DP_BOUNDARY_INVERSE, DP_BOUNDARY_MASK, check

DIRECTIONS = ("left", "top", "right", "bottom")
COUNTS = ("both", "target", "predicted")
MAX_DIM, MAX_T = _lib.DP_BOUNDARY_MAX_DIM, _lib.DP_BOUNDARY_MAX_T
_WHERE = "the boundary metric runs on the ROCm device (csrc/dp_boundary.hip)"


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.DPError(_WHERE)
    return torch.device("cuda", torch.cuda.current_device())


_NUMPY = {torch.float32: np.float32, torch.bool: np.bool_, torch.uint8: np.uint8}


def _typed(a, what: str, dtypes) -> None:
    """ValueError unless `a` is a 2-D tensor or numpy array of one of `dtypes` with sides in [1, MAX_DIM]."""
    if not torch.is_tensor(a) and not isinstance(a, np.ndarray):
        raise ValueError(f"{what} must be a tensor or a numpy array")
    if a.ndim != 2:
        raise ValueError(f"{what} must be 2-D (got {a.ndim}-D)")
    ok = a.dtype in dtypes if torch.is_tensor(a) else a.dtype.type in [_NUMPY[d] for d in dtypes]
    if not ok:
        raise ValueError(f"{what} must be {' / '.join(str(d) for d in dtypes)} (got {a.dtype})")
    h, w = a.shape
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise ValueError(f"{what}: sides must be in [1, {MAX_DIM}] (got {h} x {w})")


def _on_device(a, device=None) -> torch.Tensor:
    """A checked image as a device tensor with unit column stride (rows may be strided): a numpy array is uploaded
    (to `device`, or the current one), a host tensor is refused."""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a)).to(device if device is not None and device.type == "cuda" else _device())
    if a.device.type != "cuda":
        raise _lib.DPError(_WHERE)
    if a.stride(1) != 1 or a.stride(0) < a.shape[1]:
        a = a.contiguous()
    return a


def _device_of(*images):
    for a in images:
        if torch.is_tensor(a):
            return a.device
    return None


_DEPTH, _MASK = (torch.float32,), (torch.bool, torch.uint8, torch.float32)


def _thresholds(thresholds) -> np.ndarray:
    th = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if not 1 <= th.size <= MAX_T:
        raise ValueError(f"between 1 and {MAX_T} thresholds (got {th.size})")
    if not np.isfinite(th).all():
        raise ValueError("thresholds must be finite")
    return th


def boundary_counts(pred, target, thresholds, kind: int = DP_BOUNDARY_DEPTH) -> torch.Tensor:
    """Device uint64 [n, 4, 3]: per threshold and direction (`DIRECTIONS`) the cells that are an edge of both images, of
    the target, of the prediction (`COUNTS`), from `dp_boundary_counts`.  `kind` DP_BOUNDARY_DEPTH: `target` is a float32
    depth and both sides' edges are plain (the F1 case); DP_BOUNDARY_MASK: `target` is a mask (bool, uint8 or float32,
    non-zero = set) and the prediction's edges are thinned (the recall case); | DP_BOUNDARY_INVERSE: the depths are
    inverse depths already.  A ratio meets a threshold as (double)ratio > t.  Asynchronous, no read-back."""
    k = int(kind)
    if k & ~DP_BOUNDARY_INVERSE not in (DP_BOUNDARY_DEPTH, DP_BOUNDARY_MASK) or k < 0:
        raise ValueError(f"unknown kind {kind}")
    is_mask = (k & ~DP_BOUNDARY_INVERSE) == DP_BOUNDARY_MASK
    _typed(pred, "the predicted depth", _DEPTH)
    _typed(target, "the target mask" if is_mask else "the target depth", _MASK if is_mask else _DEPTH)
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"prediction {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    th = _thresholds(thresholds)
    p = _on_device(pred, _device_of(pred, target))
    t = _on_device(target, p.device)
    if t.device != p.device:
        raise ValueError("prediction and target must be on one device")
    if is_mask and t.dtype != torch.uint8:
        t = (t != 0).to(torch.uint8)
    lib = _lib.load()
    h, w = p.shape
    out = torch.empty((th.size, 4, 3), dtype=torch.uint64, device=p.device)
    ws = torch.empty(int(lib.dp_boundary_workspace_size(h, w, th.size)), dtype=torch.uint8, device=p.device)
    check(lib.dp_boundary_counts(p.data_ptr(), p.stride(0), t.data_ptr(), t.stride(0), k, h, w,
                                 th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), th.size, out.data_ptr(), ws.data_ptr(),
                                 ws.numel(), torch.cuda.current_stream(p.device).cuda_stream), "dp_boundary_counts")
    return out


def boundary_edges(depth, t: float, thinned: bool = False) -> torch.Tensor:
    """Device uint8 [4, H, W]: the (left, top, right, bottom) edge maps of a float32 depth at threshold `t`
    (`dp_boundary_edges`), the reference's fgbg_depth or, `thinned`, fgbg_depth_thinned of the inverse depth; 0 outside
    each map's extent (the last column of left / right, the last row of top / bottom).  (double)ratio > t."""
    _typed(depth, "the depth", _DEPTH)
    if not np.isfinite(float(t)):
        raise ValueError("the threshold must be finite")
    d = _on_device(depth)
    lib = _lib.load()
    h, w = d.shape
    out = torch.empty((4, h, w), dtype=torch.uint8, device=d.device)
    ws = torch.empty(int(lib.dp_boundary_workspace_size(h, w, 1)), dtype=torch.uint8, device=d.device)
    check(lib.dp_boundary_edges(d.data_ptr(), d.stride(0), h, w, float(t), int(bool(thinned)), out.data_ptr(), ws.data_ptr(),
                                ws.numel(), torch.cuda.current_stream(d.device).cuda_stream), "dp_boundary_edges")
    return out


def _host_counts(counts: torch.Tensor) -> list:
    """[n][4][3] Python ints (the one read-back of a score)."""
    return counts.view(torch.int64).cpu().numpy().tolist()


def recall_from_counts(c) -> float:
    """The reference's recall expression on one threshold's [4][3] counts."""
    return 0.25 * (c[0][0] / max(c[0][1], 1) + c[1][0] / max(c[1][1], 1) + c[2][0] / max(c[2][1], 1) + c[3][0] / max(c[3][1], 1))


def precision_from_counts(c) -> float:
    return 0.25 * (c[0][0] / max(c[0][2], 1) + c[1][0] / max(c[1][2], 1) + c[2][0] / max(c[2][2], 1) + c[3][0] / max(c[3][2], 1))


def f1_from_counts(c, return_p: bool = False, return_r: bool = False) -> float:
    r, p = recall_from_counts(c), precision_from_counts(c)
    if r + p == 0:
        return 0.0
    if return_p:
        return p
    if return_r:
        return r
    return 2 * (r * p) / (r + p)


def weighted_score(counts, thresholds, kind: int) -> float:
    """The weighted score of host counts [n][4][3] (F1 for DP_BOUNDARY_DEPTH, recall for DP_BOUNDARY_MASK) with the weights
    thresholds / thresholds.sum(), summed by numpy as the reference does."""
    th = np.asarray(thresholds, dtype=np.float64)
    one = recall_from_counts if int(kind) == DP_BOUNDARY_MASK else f1_from_counts
    return np.sum(np.array([one(c) for c in counts]) * (th / th.sum()))


def boundary_f1(pr, gt, t: float, return_p: bool = False, return_r: bool = False) -> float:
    """Boundary F1 (or precision / recall) at one threshold.  As in the reference, `pr` and `gt` are INVERSE depths
    (float32), compared as (double)ratio > t."""
    c = _host_counts(boundary_counts(pr, gt, [float(t)], DP_BOUNDARY_DEPTH | DP_BOUNDARY_INVERSE))[0]
    return f1_from_counts(c, return_p, return_r)


def edge_recall_matting(pr, gt, t: float) -> float:
    """Edge recall at one threshold.  As in the reference, `pr` is an INVERSE depth (float32) and `gt` a bool mask; `t`
    is a weak scalar there, so the ratio is compared with np.float32(t)."""
    if (torch.is_tensor(gt) and gt.dtype != torch.bool) or (isinstance(gt, np.ndarray) and gt.dtype != np.bool_):
        raise ValueError("the mask must be bool")
    c = _host_counts(boundary_counts(pr, gt, [float(np.float32(t))], DP_BOUNDARY_MASK | DP_BOUNDARY_INVERSE))[0]
    return recall_from_counts(c)


def get_thresholds_and_weights(t_min: float, t_max: float, N: int) -> Tuple[np.ndarray, np.ndarray]:
    if int(N) < 1:
        raise ValueError(f"N must be >= 1 (got {N})")
    thresholds = np.linspace(t_min, t_max, int(N))
    weights = thresholds / thresholds.sum()
    return thresholds, weights


def invert_depth(depth, eps: float = 1e-6):
    """1 / max(depth, eps) with numpy's clip rule (a NaN stays), on a numpy array or a tensor."""
    if torch.is_tensor(depth):
        return 1.0 / torch.where(depth < eps, torch.full_like(depth, eps), depth)
    return 1.0 / depth.clip(min=eps)


def _score_counts(predicted_depth, target, t_min, t_max, N, kind, alpha_threshold=None):
    if int(N) > MAX_T:
        raise ValueError(f"N must be <= {MAX_T} (got {N})")
    thresholds, _ = get_thresholds_and_weights(t_min, t_max, N)
    passed = thresholds
    if kind == DP_BOUNDARY_MASK:
        _typed(predicted_depth, "the predicted depth", _DEPTH)
        _typed(target, "the target mask", _MASK)
        target = _on_device(target, _device_of(predicted_depth, target))
        # numpy compares a float32 array with float32(alpha_threshold) (a weak Python scalar); the same number either way
        target = target > (float(np.float32(alpha_threshold)) if target.dtype == torch.float32 else alpha_threshold)
        passed = thresholds.astype(np.float32).astype(np.float64)          # the reference's float(t) meets float32 ratios
    return thresholds, boundary_counts(predicted_depth, target, passed, kind)


def SI_boundary_F1(predicted_depth, target_depth, t_min: float = 1.05, t_max: float = 1.25, N: int = 10) -> float:
    """Scale-invariant boundary F1 of a predicted and a target depth (2-D float32, device tensors or numpy arrays)."""
    thresholds, counts = _score_counts(predicted_depth, target_depth, t_min, t_max, N, DP_BOUNDARY_DEPTH)
    return weighted_score(_host_counts(counts), thresholds, DP_BOUNDARY_DEPTH)


def SI_boundary_Recall(predicted_depth, target_mask, t_min: float = 1.05, t_max: float = 1.25, N: int = 10,
                       alpha_threshold: float = 0.1) -> float:
    """Scale-invariant boundary recall of a predicted depth (2-D float32) against a mask (bool, uint8 or float32 alpha,
    set where > alpha_threshold)."""
    thresholds, counts = _score_counts(predicted_depth, target_mask, t_min, t_max, N, DP_BOUNDARY_MASK, alpha_threshold)
    return weighted_score(_host_counts(counts), thresholds, DP_BOUNDARY_MASK)

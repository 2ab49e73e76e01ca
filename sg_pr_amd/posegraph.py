"""Planar pose-graph relaxation over accepted loop closures (include/sgpr_posegraph.h).

The entry points are declared in the second public header; this module has engine.bind_header parse it and set the
signatures on the library engine.load_library() returns - there is no table of them in Python.  No CPU fallback.
"""
import os

import numpy as np
import torch

from . import _build, engine

HEADER = os.path.join(_build.REPO, "include", "sgpr_posegraph.h")
_ABI = engine.public_header(os.path.basename(HEADER))
_C = _ABI.constants

ABI_SYMBOLS = [name for name, _, _ in _ABI.functions]
MAX_SCANS, MAX_CLOSURES, MAX_ITERS = (_C["SGPR_POSEGRAPH_" + n] for n in ("MAX_SCANS", "MAX_CLOSURES", "MAX_ITERS"))
SEGMENT = _C["SGPR_POSEGRAPH_SEGMENT"]
NONFINITE, NO_ANCHOR, DEGENERATE = (_C["SGPR_POSEGRAPH_" + n] for n in ("NONFINITE", "NO_ANCHOR", "DEGENERATE"))
CONVERGED, STOP_MAX_ITERS, BREAKDOWN = (_C["SGPR_POSEGRAPH_" + n] for n in ("CONVERGED", "STOP_MAX_ITERS", "BREAKDOWN"))
STOP_NAMES = {CONVERGED: "converged", STOP_MAX_ITERS: "max_iters", BREAKDOWN: "breakdown"}
# 1 / sigma^2 of synth.drift_world's odometry steps (0.004 rad, 0.03 m) and closures (0.01 rad, 0.15 m)
W_ODO, W_CLO = (62500.0, 1100.0), (10000.0, 44.0)


def load_library():
    """engine.load_library() with the signatures of include/sgpr_posegraph.h set on it"""
    engine.bind_header(os.path.basename(HEADER))
    return engine.load_library()


def workspace_bytes(m, c):
    return int(load_library().sgpr_posegraph_optimize_workspace_bytes(int(m), int(c)))


def info_dict(info, resid):
    """the int32 [8] / float64 [4] outputs of sgpr_posegraph_optimize (host arrays) as a dict"""
    info, resid = np.asarray(info).reshape(8), np.asarray(resid, dtype=np.float64).reshape(4)
    return {"status": int(info[0]), "iterations": (int(info[1]), int(info[2])),
            "stop": (STOP_NAMES.get(int(info[3]), "?"), STOP_NAMES.get(int(info[4]), "?")),
            "live_closures": int(info[5]), "free_scans": int(info[6]), "active_sessions": int(info[7]),
            "rz0": (float(resid[0]), float(resid[2])), "rz": (float(resid[1]), float(resid[3])),
            "info": info.copy(), "resid": resid.copy()}


def optimize_async(X, rows, cols, T, starts=None, fixed=None, weight=None, w_odo=W_ODO, w_clo=W_CLO, max_iters=1000,
                   rel_tol=1e-9, device=None, workspace=None):
    """sgpr_posegraph_optimize without reading anything back -> (X_out f64 [M,4], info i32 [8], resid f64 [4]) device
    tensors, asynchronous on the current stream.  workspace: a uint8 device tensor to carve (any contents), or None."""
    lib = load_library()
    if device is None:
        device = engine._device_of(X, T, rows, cols)
    x = engine._on(X, device, torch.float64).view(-1, 4)
    r, c = (engine._on(t, device, torch.int32).view(-1) for t in (rows, cols))
    t = engine._on(T, device, torch.float64).view(-1, 4)
    m, n = x.shape[0], r.numel()
    if c.numel() != n or t.shape[0] != n:
        raise ValueError("posegraph.optimize: rows, cols and T must describe the same number of closures")
    wgt = None if weight is None else engine._on(weight, device, torch.float64).view(-1)
    if wgt is not None and wgt.numel() != n:
        raise ValueError("posegraph.optimize: weight must hold one multiplier per closure")
    fx = None if fixed is None else engine._on(torch.as_tensor(fixed).to(torch.bool), device, torch.uint8).view(-1)
    if fx is not None and fx.numel() != m:
        raise ValueError("posegraph.optimize: fixed must hold one entry per scan")
    table = engine._session_table(starts)
    out = torch.empty_like(x)
    info = torch.empty(8, dtype=torch.int32, device=device)
    resid = torch.empty(4, dtype=torch.float64, device=device)
    need = workspace_bytes(m, n) if 0 <= m <= MAX_SCANS and 0 <= n <= MAX_CLOSURES else 0
    ws = workspace if workspace is not None else torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        engine._check(lib.sgpr_posegraph_optimize(
            engine._ptr(x), m, *engine._table_args(table),
            engine._ptr(r), engine._ptr(c), engine._ptr(t), engine._ptr(wgt), n, engine._ptr(fx), float(w_odo[0]),
            float(w_odo[1]), float(w_clo[0]), float(w_clo[1]), int(max_iters), float(rel_tol), engine._ptr(out),
            engine._ptr(info), engine._ptr(resid), engine._ptr(ws), ws.numel(), engine._stream(device)))
    if m == 0:
        info.zero_()
        resid.zero_()
    return out, info, resid


def optimize(X, rows, cols, T, starts=None, fixed=None, weight=None, w_odo=W_ODO, w_clo=W_CLO, max_iters=1000,
             rel_tol=1e-9, device=None):
    """One map in one frame from the stacked planar odometry X [M,4] (c, s, x, y; metrics.planar_odometry) of a map
    with session table `starts` and the closures (rows[p], cols[p], T[p] = the refined transform of verify_pairs: a point
    of scan rows[p] into scan cols[p]) - rotations, then translations, by preconditioned conjugate gradients on the
    device.  fixed: a mask of the scans that keep their pose (None = scan 0); weight: a multiplier per closure;
    w_odo / w_clo: (rotation, translation) weights of an odometry step and of a closure.
    -> (X_out f64 [M,4] device tensor, info dict: status, iterations (R, T), stop (R, T), live_closures, free_scans,
    active_sessions, rz0, rz).  Reading the info synchronises the stream."""
    out, info, resid = optimize_async(X, rows, cols, T, starts, fixed, weight, w_odo, w_clo, max_iters, rel_tol, device)
    return out, info_dict(info.cpu().numpy(), resid.cpu().numpy())

"""Localise scans in the map: pose consensus over verified candidates (include/sgpr_localize.h).

The entry point is declared in the third public header; this module has engine.bind_header parse it and set the
signature on the library engine.load_library() returns - there is no table of them in Python.  No CPU fallback.
"""
import math
import os

import torch

from . import _build, engine

HEADER = os.path.join(_build.REPO, "include", "sgpr_localize.h")
_ABI = engine.public_header(os.path.basename(HEADER))
_C = _ABI.constants

ABI_SYMBOLS = [name for name, _, _ in _ABI.functions]
MAX_K, MAX_LEN = _C["SGPR_LOCALIZE_MAX_K"], _C["SGPR_LOCALIZE_MAX_LEN"]
NO_HYPOTHESIS, DEGENERATE = _C["SGPR_LOCALIZE_NO_HYPOTHESIS"], _C["SGPR_LOCALIZE_DEGENERATE"]


def load_library():
    """engine.load_library() with the signatures of include/sgpr_localize.h set on it"""
    engine.bind_header(os.path.basename(HEADER))
    return engine.load_library()


def localize_async(map_poses, cols, T, accept=None, odo=None, starts=None, seq_len=1, max_trans=1.0, max_yaw=0.1,
                   device=None):
    """sgpr_localize_scans without reading anything back -> (pose f64 [Q,4], stat i32 [Q,4] = (support, live slots,
    winner slot, flags), spread f64 [Q]) device tensors, asynchronous on the current stream."""
    lib = load_library()
    if device is None:
        device = engine._device_of(map_poses, T, cols, odo)
    x = engine._on(map_poses, device, torch.float64).view(-1, 4)
    c = engine._on(cols, device, torch.int32)
    if c.dim() != 2:
        raise ValueError("localize: cols must be [Q, K]")
    q, k = c.shape
    t = engine._on(T, device, torch.float64)
    if t.numel() != q * k * 4:
        raise ValueError("localize: T must hold one transform (c, s, x, y) per candidate")
    acc = None if accept is None else engine._on(torch.as_tensor(accept).to(torch.bool), device, torch.uint8)
    if acc is not None and acc.numel() != q * k:
        raise ValueError("localize: accept must hold one entry per candidate")
    od = None if odo is None else engine._on(odo, device, torch.float64).view(-1, 4)
    if od is not None and od.shape[0] != q:
        raise ValueError("localize: odo must hold one pose per query")
    table = engine._session_table(starts)
    m = x.shape[0]
    if m == 0:
        x = torch.zeros(1, 4, dtype=torch.float64, device=device)       # (a pointer to pass: no row of it is read)
    pose = torch.empty(q, 4, dtype=torch.float64, device=device)
    stat = torch.empty(q, 4, dtype=torch.int32, device=device)
    spread = torch.empty(q, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        engine._check(lib.sgpr_localize_scans(
            engine._ptr(x), m, engine._ptr(c), engine._ptr(t), engine._ptr(acc), q, k, engine._ptr(od),
            *engine._table_args(table), int(seq_len),
            float(max_trans), math.cos(float(max_yaw)), engine._ptr(pose), engine._ptr(stat), engine._ptr(spread),
            engine._stream(device)))
    return pose, stat, spread


def localize(map_poses, cols, T, accept=None, odo=None, starts=None, seq_len=1, max_trans=1.0, max_yaw=0.1, device=None,
             min_support=None):
    """Where is every query scan in the map?  map_poses [M,4]: planar poses (c, s, x, y) of the map scans; cols [Q,K]:
    the candidate map scans of every query (outside 0..M-1 = padding); T [Q,K,4]: the refined transform of verify_pairs
    (a point of the query scan into the candidate); accept [Q,K]: which candidates take part (None: all); odo [Q,4]: the
    query drive's own planar odometry (needed for seq_len > 1) and starts its session table.  Every candidate of the
    last seq_len scans of a query's session, carried forward by the odometry, is a hypothesis of the query's pose; the
    answer is the mean of the largest set that agrees with one of them within max_trans metres and max_yaw radians.
    -> dict of device tensors: pose f64 [Q,4] (NaN without a live hypothesis), support, live, winner, flags i32 [Q],
    spread f64 [Q] (RMS distance of the supporters to the mean, m); with min_support also accept bool [Q] =
    support >= min_support."""
    pose, stat, spread = localize_async(map_poses, cols, T, accept, odo, starts, seq_len, max_trans, max_yaw, device)
    out = {"pose": pose, "support": stat[:, 0], "live": stat[:, 1], "winner": stat[:, 2], "flags": stat[:, 3],
           "spread": spread}
    if min_support is not None:
        out["accept"] = out["support"] >= int(min_support)
    return out

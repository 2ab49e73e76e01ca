"""The semantic landmark map: the nodes of every scan fused in the map frame (include/sgpr_landmarks.h),
the refinement of the poses on that map (include/sgpr_landmark_refine.h), the alignment of further
scans to it (include/sgpr_landmark_align.h), the folding of aligned scans into it
(include/sgpr_landmark_update.h), the tallies of what a drive should have seen of it and did see
(include/sgpr_landmark_persist.h), the tracking of a drive through it, scan by scan
(include/sgpr_landmark_track.h), the relocalisation of a scan in it with no prior pose
(include/sgpr_landmark_relocalize.h) and the joining and compaction of maps on their records alone
(include/sgpr_landmark_merge.h).

The entry points are declared in the fourth to eleventh public headers; this module has engine.bind_header parse them and
set the signatures on the library engine.load_library() returns - there is no table of them in Python.  No CPU fallback.
"""
import os

import numpy as np
import torch

from . import _build, engine, synth

HEADER = os.path.join(_build.REPO, "include", "sgpr_landmarks.h")
_ABI = engine.public_header(os.path.basename(HEADER))
_C = _ABI.constants

ABI_SYMBOLS = [name for name, _, _ in _ABI.functions]
REFINE_HEADER = os.path.join(_build.REPO, "include", "sgpr_landmark_refine.h")
REFINE_ABI_SYMBOLS = [name for name, _, _ in engine.public_header(os.path.basename(REFINE_HEADER)).functions]
ALIGN_HEADER = os.path.join(_build.REPO, "include", "sgpr_landmark_align.h")
ALIGN_ABI_SYMBOLS = [name for name, _, _ in engine.public_header(os.path.basename(ALIGN_HEADER)).functions]
UPDATE_HEADER = os.path.join(_build.REPO, "include", "sgpr_landmark_update.h")
UPDATE_ABI_SYMBOLS = [name for name, _, _ in engine.public_header(os.path.basename(UPDATE_HEADER)).functions]
PERSIST_HEADER = os.path.join(_build.REPO, "include", "sgpr_landmark_persist.h")
PERSIST_ABI_SYMBOLS = [name for name, _, _ in engine.public_header(os.path.basename(PERSIST_HEADER)).functions]
TRACK_HEADER = os.path.join(_build.REPO, "include", "sgpr_landmark_track.h")
_TRACK_ABI = engine.public_header(os.path.basename(TRACK_HEADER))
TRACK_ABI_SYMBOLS = [name for name, _, _ in _TRACK_ABI.functions]
ALIGN_NONFINITE, ALIGN_KEPT = 1, 2       # flags of sgpr_landmark_align (d_stat[q][3])
_T = _TRACK_ABI.constants
TRACK_MAX_STAGES, TRACK_START_LOST = _T["SGPR_TRACK_MAX_STAGES"], _T["SGPR_TRACK_START_LOST"]
TRACK_NONFINITE, TRACK_KEPT, TRACK_LOST, TRACK_NO_ODOM, TRACK_REACQUIRE = (
    _T["SGPR_TRACK_" + k] for k in ("NONFINITE", "KEPT", "LOST", "NO_ODOM", "REACQUIRE"))   # flags of a tracked scan
RELOCALIZE_HEADER = os.path.join(_build.REPO, "include", "sgpr_landmark_relocalize.h")
_RELOC_ABI = engine.public_header(os.path.basename(RELOCALIZE_HEADER))
RELOCALIZE_ABI_SYMBOLS = [name for name, _, _ in _RELOC_ABI.functions]
_R = _RELOC_ABI.constants
RELOC_MAX_STAGES = _R["SGPR_RELOC_MAX_STAGES"]
RELOC_FOUND, RELOC_KEPT, RELOC_TRUNCATED, RELOC_NO_HYPOTHESIS = (
    _R["SGPR_RELOC_" + k] for k in ("FOUND", "KEPT", "TRUNCATED", "NO_HYPOTHESIS"))          # flags of a relocalised scan
MERGE_HEADER = os.path.join(_build.REPO, "include", "sgpr_landmark_merge.h")
MERGE_ABI_SYMBOLS = [name for name, _, _ in engine.public_header(os.path.basename(MERGE_HEADER)).functions]
MAX_LABELS = _C["SGPR_LANDMARK_MAX_LABELS"]
DEFAULT_RADIUS, DEFAULT_TAU_Z = 0.75, 0.75
DEFAULT_MAX_LANDMARKS = 1 << 22          # the default capacity is G N, capped here; build() re-runs past it
_CHUNK_BYTES = 1 << 28                   # virtual_scans: the largest Q x L float64 matrix alive


def load_library():
    """engine.load_library() with the signatures of include/sgpr_landmarks.h, include/sgpr_landmark_refine.h,
    include/sgpr_landmark_align.h, include/sgpr_landmark_update.h, include/sgpr_landmark_persist.h,
    include/sgpr_landmark_track.h, include/sgpr_landmark_relocalize.h and include/sgpr_landmark_merge.h set on it"""
    engine.bind_header(os.path.basename(HEADER))
    engine.bind_header(os.path.basename(REFINE_HEADER))
    engine.bind_header(os.path.basename(ALIGN_HEADER))
    engine.bind_header(os.path.basename(UPDATE_HEADER))
    engine.bind_header(os.path.basename(PERSIST_HEADER))
    engine.bind_header(os.path.basename(TRACK_HEADER))
    engine.bind_header(os.path.basename(RELOCALIZE_HEADER))
    engine.bind_header(os.path.basename(MERGE_HEADER))
    return engine.load_library()


def workspace_bytes(G, N):
    return int(load_library().sgpr_landmark_workspace_bytes(int(G), int(N)))


def _radius_table(radius):
    r = np.atleast_1d(np.asarray(DEFAULT_RADIUS if radius is None else radius, dtype=np.float64))
    if r.ndim != 1:
        raise ValueError("landmarks: radius is a scalar or one value per label")
    if r.size == 1:
        r = np.full(synth.NUM_LABELS, r[0], dtype=np.float64)
    return np.ascontiguousarray(r)


def build_async(centers, labels, poses, starts=None, radius=None, tau_z=DEFAULT_TAU_Z, max_landmarks=None, workspace=None,
                device=None):
    """sgpr_landmark_map without reading anything back -> dict of device tensors, asynchronous on the current stream:
    center f64 [max_landmarks,3], label, count, first i32 [max_landmarks], sessions i64 [max_landmarks] (the bits of the
    uint64 mask), spread f64 [max_landmarks], node_landmark i32 [G,N], num i32 [2] = (landmarks found, live nodes).
    Only the first min(num[0], max_landmarks) records are written.  workspace: a uint8 device tensor of at least
    workspace_bytes(G, N) to reuse (None: one is allocated)."""
    lib = load_library()
    if device is None:
        device = engine._device_of(centers, labels, poses)
    lab = engine._on(labels, device, torch.int32)
    if lab.dim() != 2:
        raise ValueError("landmarks: labels must be [G, N]")
    g, n = lab.shape
    cen = engine._on(centers, device, torch.float32)
    if cen.numel() != g * n * 3:
        raise ValueError("landmarks: centers must be [G, N, 3]")
    x = engine._on(poses, device, torch.float64)
    if x.numel() != g * 4:
        raise ValueError("landmarks: poses must hold one planar pose (c, s, x, y) per scan")
    table = engine._session_table(starts)
    rad = _radius_table(radius)
    cap = min(g * n, DEFAULT_MAX_LANDMARKS) if max_landmarks is None else int(max_landmarks)
    rows = max(cap, 0)
    out = {"center": torch.empty(rows, 3, dtype=torch.float64, device=device),
           "label": torch.empty(rows, dtype=torch.int32, device=device),
           "count": torch.empty(rows, dtype=torch.int32, device=device),
           "first": torch.empty(rows, dtype=torch.int32, device=device),
           "sessions": torch.empty(rows, dtype=torch.int64, device=device),
           "spread": torch.empty(rows, dtype=torch.float64, device=device),
           "node_landmark": torch.empty(g, n, dtype=torch.int32, device=device),
           "num": torch.zeros(2, dtype=torch.int32, device=device)}       # (G N == 0: the call writes nothing)
    need = workspace_bytes(g, n)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    elif workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("landmarks: the workspace must be a contiguous uint8 tensor on %s" % (device,))
    with torch.cuda.device(device):
        engine._check(lib.sgpr_landmark_map(
            engine._ptr(cen), engine._ptr(lab), g, n, engine._ptr(x),
            *engine._table_args(table),
            rad.ctypes.data, rad.shape[0], float(tau_z), cap, engine._ptr(out["center"]), engine._ptr(out["label"]),
            engine._ptr(out["count"]), engine._ptr(out["first"]), engine._ptr(out["sessions"]),
            engine._ptr(out["spread"]), engine._ptr(out["node_landmark"]), engine._ptr(out["num"]),
            engine._ptr(workspace), workspace.numel(), engine._stream(device)))
    return out


def build(centers, labels, poses, starts=None, radius=None, tau_z=DEFAULT_TAU_Z, max_landmarks=None, workspace=None,
          device=None):
    """The landmark map of G scans.  centers f32 [G,N,3], labels i32 [G,N]: the packed node arrays (label -1 =
    padding); poses [G,4]: planar (c, s, x, y), a scan point into the map frame; starts: the session table of the scans
    (None: one session); radius: the link radius in metres, a scalar (for every label of synth.NUM_LABELS) or one value
    per label (0 = the label takes no part); tau_z: the height tolerance.  Nodes of one label within the radius link;
    a landmark is a connected component, numbered by its lowest node g N + n.
    -> dict of device tensors trimmed to the landmarks found: center f64 [L,3], label, count, first i32 [L], sessions
    i64 [L] (bit j = seen by session j), spread f64 [L] (planar RMS distance of the observations to the centre, m),
    node_landmark i32 [G,N] (-1 = dead node); num_landmarks, live_nodes int.  If max_landmarks (default G N, capped at
    DEFAULT_MAX_LANDMARKS) was too small the call is repeated once with the reported count."""
    kw = dict(starts=starts, radius=radius, tau_z=tau_z, workspace=workspace, device=device)
    out = build_async(centers, labels, poses, max_landmarks=max_landmarks, **kw)
    found, live = (int(v) for v in out["num"].tolist())
    if found > out["label"].shape[0]:
        out = build_async(centers, labels, poses, max_landmarks=found, **kw)
    res = {k: out[k][:found] for k in ("center", "label", "count", "first", "sessions", "spread")}
    res["node_landmark"] = out["node_landmark"]
    res["num_landmarks"], res["live_nodes"] = found, live
    return res


def _popcount64(words):
    w = torch.as_tensor(words).to(torch.int64)
    n = torch.zeros_like(w)
    for b in range(64):
        n += (w >> b) & 1
    return n


def select(lm, min_count=1, min_sessions=1, keep=None):
    """mask bool [L] of the landmarks with at least min_count observations, seen by at least min_sessions sessions; keep:
    a further mask over the landmarks that is ANDed in, e.g. persist's (None: none)"""
    count = torch.as_tensor(lm["count"])
    mask = (count >= int(min_count)) & (_popcount64(lm["sessions"]).to(count.device) >= int(min_sessions))
    if keep is not None:
        more = torch.as_tensor(keep).to(count.device).reshape(-1) != 0
        if more.numel() != mask.numel():
            raise ValueError("landmarks.select: keep must hold one entry per landmark")
        mask = mask & more
    return mask


def refine_workspace_bytes(G, N, L):
    return int(load_library().sgpr_landmark_refine_workspace_bytes(int(G), int(N), int(L)))


def refine_async(centers, labels, poses, lm, use=None, fixed=None, iters=10, min_nodes=6, workspace=None, device=None):
    """sgpr_landmark_refine without reading anything back -> dict of device tensors, asynchronous on the current stream:
    poses f64 [G,4], cost f64 [iters+1], info i32 [4] = (used nodes and landmarks observed at the end, scans the last fit
    re-fitted, free scans it kept).  centers f32 [G,N,3], labels i32 [G,N] (its shape is all that is read: the landmark
    of a node decides), poses [G,4] planar; lm: the dict of build / build_async made on THOSE poses ("node_landmark",
    and "count" for the number of landmarks); use: a mask over the landmarks (select makes one; None: all of them);
    fixed: a mask over the scans that keep their pose (None: no scan).  workspace: a uint8 device tensor of at least
    refine_workspace_bytes(G, N, L) to reuse."""
    lib = load_library()
    if device is None:
        device = engine._device_of(centers, poses, lm["node_landmark"])
    node = engine._on(lm["node_landmark"], device, torch.int32)
    if node.dim() != 2 or tuple(node.shape) != tuple(torch.as_tensor(labels).shape):
        raise ValueError("landmarks.refine: node_landmark and labels must be [G, N]")
    g, n = node.shape
    cen = engine._on(centers, device, torch.float32)
    if cen.numel() != g * n * 3:
        raise ValueError("landmarks.refine: centers must be [G, N, 3]")
    x = engine._on(poses, device, torch.float64)
    if x.numel() != g * 4:
        raise ValueError("landmarks.refine: poses must hold one planar pose (c, s, x, y) per scan")
    n_lm = int(torch.as_tensor(lm["count"]).shape[0])
    if use is None:
        mask = torch.ones(n_lm, dtype=torch.uint8, device=device)
    else:
        mask = engine._on(torch.as_tensor(use).reshape(-1) != 0, device, torch.bool).to(torch.uint8)
        if mask.numel() != n_lm:
            raise ValueError("landmarks.refine: use must hold one entry per landmark")
    fix = None
    if fixed is not None:
        fix = engine._on(torch.as_tensor(fixed).reshape(-1) != 0, device, torch.bool).to(torch.uint8)
        if fix.numel() != g:
            raise ValueError("landmarks.refine: fixed must hold one entry per scan")
    t = int(iters)
    out = {"poses": torch.empty(g, 4, dtype=torch.float64, device=device),
           "cost": torch.full((max(t, 0) + 1,), float("nan"), dtype=torch.float64, device=device),
           "info": torch.zeros(4, dtype=torch.int32, device=device)}          # (G N == 0: the call writes nothing)
    need = refine_workspace_bytes(g, n, n_lm)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    elif workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("landmarks.refine: the workspace must be a contiguous uint8 tensor on %s" % (device,))
    with torch.cuda.device(device):
        engine._check(lib.sgpr_landmark_refine(
            engine._ptr(cen), g, n, engine._ptr(x), engine._ptr(node), engine._ptr(mask), n_lm, engine._ptr(fix), t,
            int(min_nodes), engine._ptr(out["poses"]), engine._ptr(out["cost"]), engine._ptr(out["info"]),
            engine._ptr(workspace), workspace.numel(), engine._stream(device)))
    if g * n == 0:
        out["poses"].copy_(x.reshape(g, 4))
    return out


def refine(centers, labels, poses, lm, use=None, fixed=None, iters=10, min_nodes=6, workspace=None, device=None):
    """Refine the planar poses of G scans on the landmark map `lm` that build made on them: `iters`
    alternations of "a landmark's centre is the mean of its observations" and "every scan is re-fitted rigidly to the
    centres of its nodes' landmarks", all scans of a step against the same centres.  Arguments as refine_async; a scan
    with fewer than min_nodes nodes on the landmarks in use keeps its pose.
    -> (poses f64 [G,4] on the device, info dict: cost (numpy float64 [iters+1], the RMS distance in metres of the
    observations to their centres before every step and at the end), used_nodes, landmarks, refitted, kept)."""
    out = refine_async(centers, labels, poses, lm, use=use, fixed=fixed, iters=iters, min_nodes=min_nodes,
                       workspace=workspace, device=device)
    used, seen, refit, kept = (int(v) for v in out["info"].tolist())
    return out["poses"], {"cost": out["cost"].cpu().numpy(), "used_nodes": used, "landmarks": seen, "refitted": refit,
                          "kept": kept}


def align_workspace_bytes(Q, N, L):
    return int(load_library().sgpr_landmark_align_workspace_bytes(int(Q), int(N), int(L)))


def align_async(centers, labels, poses, lm, use=None, radius=None, tau_z=DEFAULT_TAU_Z, iters=10, min_nodes=6, workspace=None,
                device=None):
    """sgpr_landmark_align without reading anything back -> dict of device tensors, asynchronous on the current stream:
    poses f64 [Q,4], node_landmark i32 [Q,N] (the landmark of a node, -2 = live without one, -1 = dead), stat i32 [Q,4] =
    (matched, live, steps that re-fitted, flags: ALIGN_NONFINITE, ALIGN_KEPT), rms f64 [Q].  centers f32 [Q,N,3], labels
    i32 [Q,N]: the query scans, which need not be part of the map; poses [Q,4]: their approximate planar poses in the
    map frame; lm: the dict of build / build_async ("center", "label"); use: a mask over the landmarks (select makes
    one; None: all of them); radius: the gate in metres, a scalar or one value per label; tau_z: the height tolerance.
    workspace: a uint8 device tensor of at least align_workspace_bytes(Q, N, L) to reuse."""
    lib = load_library()
    if device is None:
        device = engine._device_of(centers, labels, poses, lm["center"])
    lab = engine._on(labels, device, torch.int32)
    if lab.dim() != 2:
        raise ValueError("landmarks.align: labels must be [Q, N]")
    q, n = lab.shape
    cen = engine._on(centers, device, torch.float32)
    if cen.numel() != q * n * 3:
        raise ValueError("landmarks.align: centers must be [Q, N, 3]")
    x = engine._on(poses, device, torch.float64)
    if x.numel() != q * 4:
        raise ValueError("landmarks.align: poses must hold one planar pose (c, s, x, y) per scan")
    lm_c = engine._on(lm["center"], device, torch.float64)
    lm_l = engine._on(lm["label"], device, torch.int32)
    n_lm = int(lm_l.numel())
    if lm_c.numel() != 3 * n_lm:
        raise ValueError("landmarks.align: the map must hold center [L,3] and label [L]")
    mask = None
    if use is not None:
        mask = engine._on(torch.as_tensor(use).reshape(-1) != 0, device, torch.bool).to(torch.uint8)
        if mask.numel() != n_lm:
            raise ValueError("landmarks.align: use must hold one entry per landmark")
    rad = _radius_table(radius)
    out = {"poses": torch.empty(q, 4, dtype=torch.float64, device=device),
           "node_landmark": torch.full((q, n), -1, dtype=torch.int32, device=device),
           "stat": torch.zeros(q, 4, dtype=torch.int32, device=device),
           "rms": torch.full((q,), float("nan"), dtype=torch.float64, device=device)}   # (Q N == 0: the call writes nothing)
    need = align_workspace_bytes(q, n, n_lm)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    elif workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("landmarks.align: the workspace must be a contiguous uint8 tensor on %s" % (device,))
    with torch.cuda.device(device):
        engine._check(lib.sgpr_landmark_align(
            engine._ptr(cen), engine._ptr(lab), q, n, engine._ptr(x), engine._ptr(lm_c) if n_lm else None,
            engine._ptr(lm_l) if n_lm else None, engine._ptr(mask) if n_lm else None, n_lm, rad.ctypes.data, rad.shape[0],
            float(tau_z), int(iters), int(min_nodes), engine._ptr(out["poses"]), engine._ptr(out["node_landmark"]),
            engine._ptr(out["stat"]), engine._ptr(out["rms"]), engine._ptr(workspace), workspace.numel(),
            engine._stream(device)))
    if q * n == 0:
        out["poses"].copy_(x.reshape(q, 4))
    return out


def align(centers, labels, poses, lm, use=None, radius=None, tau_z=DEFAULT_TAU_Z, iters=10, min_nodes=6, workspace=None,
          device=None):
    """Align Q scans to the landmark map `lm` from approximate poses: `iters` rounds of "every node takes
    the nearest landmark of its label within `radius`" and "the scan is re-fitted rigidly to its matches"; every scan on
    its own.  Arguments as align_async; a scan with fewer than min_nodes matches keeps its pose.  One call converges
    inside its gate only: SG.align_to_map runs a schedule of gates.
    -> (poses f64 [Q,4] on the device, info dict of numpy arrays: matched, live, steps, flags i32 [Q], rms f64 [Q] (the
    planar RMS distance of the matched nodes to their landmarks, NaN without one), node_landmark i32 [Q,N] (-2 = a live
    node no landmark of the map explains, -1 = a dead node))."""
    out = align_async(centers, labels, poses, lm, use=use, radius=radius, tau_z=tau_z, iters=iters, min_nodes=min_nodes,
                      workspace=workspace, device=device)
    stat = out["stat"].cpu().numpy()
    return out["poses"], {"matched": stat[:, 0], "live": stat[:, 1], "steps": stat[:, 2], "flags": stat[:, 3],
                          "rms": out["rms"].cpu().numpy(), "node_landmark": out["node_landmark"].cpu().numpy()}


def track_workspace_bytes(Q, N, L, n_stages):
    return int(load_library().sgpr_landmark_track_workspace_bytes(int(Q), int(N), int(L), int(n_stages)))


def _stage_table(radii, reacquire_radii):
    """the stages of a tracking call: reacquire_radii in front of radii, each entry a scalar or one value per label ->
    (float64 [n_stages, n_labels] C-contiguous, n_reacquire)"""
    def stages(v):
        return [] if v is None else (list(v) if hasattr(v, "__len__") else [v])
    front, rest = stages(reacquire_radii), stages(radii)
    rows = [_radius_table(r) for r in front + rest]
    if not rows or len({r.shape[0] for r in rows}) != 1:
        raise ValueError("landmarks.track: every stage takes a scalar radius or one value per label, the same labels in each")
    return np.ascontiguousarray(np.stack(rows)), len(front)


def track_async(centers, labels, odom, init, lm, use=None, starts=None, radii=(2.0, DEFAULT_RADIUS), reacquire_radii=(8.0,),
                tau_z=DEFAULT_TAU_Z, iters=10, min_nodes=6, min_matched=10, max_shift=float("inf"), start_lost=False,
                workspace=None, device=None):
    """sgpr_landmark_track without reading anything back -> dict of device tensors, asynchronous on the current stream:
    poses, pred f64 [Q,4] (the tracked pose and the prediction it started from), node_landmark i32 [Q,N], stat i32 [Q,4] =
    (matched, live, steps that re-fitted, flags: TRACK_NONFINITE, TRACK_KEPT, TRACK_LOST, TRACK_NO_ODOM,
    TRACK_REACQUIRE), rms f64 [Q], num i32 [4] = (scans tracked, scans lost, longest run of lost scans, tracks).  centers
    f32 [Q,N,3], labels i32 [Q,N]: the scans of the drives, in order; odom [Q,4]: their planar poses in a frame of the
    drive's own; starts: the first scan of every track (None: one track); init [n_tracks,4]: the map-frame pose of every
    track's first scan; lm, use, tau_z, iters, min_nodes: as align_async takes them; radii: the gates every scan runs,
    reacquire_radii: the gates run in front of them after a lost scan (None or empty: none) - each a scalar or one value
    per label; a scan with fewer than min_matched matches, or fitted more than max_shift metres from its prediction, is
    lost and keeps the prediction; start_lost: the first scan of a track runs the re-acquisition gates too.  workspace: a
    uint8 device tensor of at least track_workspace_bytes(Q, N, L, n_stages) to reuse."""
    lib = load_library()
    if device is None:
        device = engine._device_of(centers, labels, odom, lm["center"])
    lab = engine._on(labels, device, torch.int32)
    if lab.dim() != 2:
        raise ValueError("landmarks.track: labels must be [Q, N]")
    q, n = lab.shape
    cen = engine._on(centers, device, torch.float32)
    if cen.numel() != q * n * 3:
        raise ValueError("landmarks.track: centers must be [Q, N, 3]")
    odo = engine._on(odom, device, torch.float64)
    if odo.numel() != q * 4:
        raise ValueError("landmarks.track: odom must hold one planar pose (c, s, x, y) per scan")
    table = engine._session_table(starts)
    n_tracks = 1 if table is None else table.shape[0]
    x0 = engine._on(init, device, torch.float64)
    if x0.numel() != n_tracks * 4:
        raise ValueError("landmarks.track: init must hold one planar pose (c, s, x, y) per track")
    lm_c = engine._on(lm["center"], device, torch.float64)
    lm_l = engine._on(lm["label"], device, torch.int32)
    n_lm = int(lm_l.numel())
    if lm_c.numel() != 3 * n_lm:
        raise ValueError("landmarks.track: the map must hold center [L,3] and label [L]")
    mask = None
    if use is not None:
        mask = engine._on(torch.as_tensor(use).reshape(-1) != 0, device, torch.bool).to(torch.uint8)
        if mask.numel() != n_lm:
            raise ValueError("landmarks.track: use must hold one entry per landmark")
    rad, n_reacquire = _stage_table(radii, reacquire_radii)
    n_stages = rad.shape[0]
    out = {"poses": torch.empty(q, 4, dtype=torch.float64, device=device),
           "pred": torch.empty(q, 4, dtype=torch.float64, device=device),
           "node_landmark": torch.full((q, n), -1, dtype=torch.int32, device=device),
           "stat": torch.zeros(q, 4, dtype=torch.int32, device=device),
           "rms": torch.full((q,), float("nan"), dtype=torch.float64, device=device),
           "num": torch.zeros(4, dtype=torch.int32, device=device)}       # (Q N == 0: the call writes nothing)
    need = track_workspace_bytes(q, n, n_lm, n_stages)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    elif workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("landmarks.track: the workspace must be a contiguous uint8 tensor on %s" % (device,))
    with torch.cuda.device(device):
        engine._check(lib.sgpr_landmark_track(
            engine._ptr(cen), engine._ptr(lab), q, n, engine._ptr(odo), *engine._table_args(table), engine._ptr(x0),
            engine._ptr(lm_c) if n_lm else None, engine._ptr(lm_l) if n_lm else None, engine._ptr(mask) if n_lm else None, n_lm,
            rad.ctypes.data, n_stages, n_reacquire, rad.shape[1], float(tau_z), int(iters), int(min_nodes), int(min_matched),
            float(max_shift), TRACK_START_LOST if start_lost else 0, engine._ptr(out["poses"]), engine._ptr(out["pred"]),
            engine._ptr(out["node_landmark"]), engine._ptr(out["stat"]), engine._ptr(out["rms"]), engine._ptr(out["num"]),
            engine._ptr(workspace), workspace.numel(), engine._stream(device)))
    if q * n == 0:
        out["poses"].zero_()
        out["pred"].zero_()
    return out


def track(centers, labels, odom, init, lm, use=None, starts=None, radii=(2.0, DEFAULT_RADIUS), reacquire_radii=(8.0,),
          tau_z=DEFAULT_TAU_Z, iters=10, min_nodes=6, min_matched=10, max_shift=float("inf"), start_lost=False, workspace=None,
          device=None):
    """Track drives through the landmark map `lm`: the scans of a track in order, each predicted from the
    tracked pose of its predecessor and the odometry between the two, then aligned to the map through the gates `radii`
    (every stage an align of that scan).  A scan that ends with fewer than min_matched matches, or more than max_shift
    from its prediction, is LOST: it keeps the prediction - the track dead-reckons on - and the next scan runs the wider
    reacquire_radii first.  Arguments as track_async.
    -> (poses f64 [Q,4] on the device, info dict of numpy arrays: pred f64 [Q,4], matched, live, steps, flags i32 [Q], lost
    bool [Q], rms f64 [Q], node_landmark i32 [Q,N] (of a lost scan too: what its last stage saw), num i32 [4] = (scans
    tracked, scans lost, longest run of lost scans, tracks))."""
    out = track_async(centers, labels, odom, init, lm, use=use, starts=starts, radii=radii, reacquire_radii=reacquire_radii,
                      tau_z=tau_z, iters=iters, min_nodes=min_nodes, min_matched=min_matched, max_shift=max_shift,
                      start_lost=start_lost, workspace=workspace, device=device)
    stat = out["stat"].cpu().numpy()
    return out["poses"], {"pred": out["pred"].cpu().numpy(), "matched": stat[:, 0], "live": stat[:, 1], "steps": stat[:, 2],
                          "flags": stat[:, 3], "lost": (stat[:, 3] & TRACK_LOST) != 0, "rms": out["rms"].cpu().numpy(),
                          "node_landmark": out["node_landmark"].cpu().numpy(), "num": out["num"].cpu().numpy()}


def relocalize_workspace_bytes(Q, N, L, n_stages):
    return int(load_library().sgpr_landmark_relocalize_workspace_bytes(int(Q), int(N), int(L), int(n_stages)))


def relocalize_async(centers, labels, lm, use=None, radius_in=None, radii=(2.0, DEFAULT_RADIUS), tau_z=DEFAULT_TAU_Z,
                     tau_edge=0.5, min_base=5.0, max_base=30.0, max_hyp=65536, min_inliers=12, sep=10.0, iters=10, min_nodes=6,
                     workspace=None, device=None):
    """sgpr_landmark_relocalize without reading anything back -> dict of device tensors, asynchronous on the current
    stream: poses, coarse, other f64 [Q,4] (the refined pose, the winning hypothesis' pose, the best hypothesis' pose at
    another place; NaN where there is none), node_landmark i32 [Q,N], stat i32 [Q,8] = (inliers, inliers of the other
    place, matched, live, steps that re-fitted, flags: RELOC_FOUND, RELOC_KEPT, RELOC_TRUNCATED, RELOC_NO_HYPOTHESIS,
    base pairs started, 0), win i32 [Q,4] = (i, i', j, j') of the winner, hypotheses i64 [Q], rms f64 [Q], num i32 [4] =
    (scans found, scans truncated, scans without a hypothesis, 0).  centers f32 [Q,N,3], labels i32 [Q,N]: the query
    scans - NO pose is taken; lm, use, tau_z, iters, min_nodes: as align_async takes them; radius_in: the inlier gate, a
    scalar or one value per label; radii: the refine stages, each a scalar or one value per label (None or empty: the
    coarse pose is returned); two nodes between min_base and max_base metres apart are laid on two landmarks of their
    labels whose distance differs by at most tau_edge; max_hyp: no further base pair is started once that many
    hypotheses are counted; a scan is found with min_inliers inliers; sep: how far another place is, metres.  workspace:
    a uint8 device tensor of at least relocalize_workspace_bytes(Q, N, L, n_stages) to reuse."""
    lib = load_library()
    if device is None:
        device = engine._device_of(centers, labels, lm["center"])
    lab = engine._on(labels, device, torch.int32)
    if lab.dim() != 2:
        raise ValueError("landmarks.relocalize: labels must be [Q, N]")
    q, n = lab.shape
    cen = engine._on(centers, device, torch.float32)
    if cen.numel() != q * n * 3:
        raise ValueError("landmarks.relocalize: centers must be [Q, N, 3]")
    lm_c = engine._on(lm["center"], device, torch.float64)
    lm_l = engine._on(lm["label"], device, torch.int32)
    n_lm = int(lm_l.numel())
    if lm_c.numel() != 3 * n_lm:
        raise ValueError("landmarks.relocalize: the map must hold center [L,3] and label [L]")
    mask = None
    if use is not None:
        mask = engine._on(torch.as_tensor(use).reshape(-1) != 0, device, torch.bool).to(torch.uint8)
        if mask.numel() != n_lm:
            raise ValueError("landmarks.relocalize: use must hold one entry per landmark")
    rad_in = _radius_table(radius_in)
    stages = [] if radii is None else (list(radii) if hasattr(radii, "__len__") else [radii])
    rows = [_radius_table(r) for r in stages]
    if any(r.shape[0] != rad_in.shape[0] for r in rows):
        raise ValueError("landmarks.relocalize: every stage takes a scalar radius or one value per label, as radius_in does")
    rad = np.ascontiguousarray(np.stack(rows)) if rows else None
    n_stages = len(rows)
    nan = float("nan")
    out = {"poses": torch.full((q, 4), nan, dtype=torch.float64, device=device),
           "coarse": torch.full((q, 4), nan, dtype=torch.float64, device=device),
           "other": torch.full((q, 4), nan, dtype=torch.float64, device=device),
           "node_landmark": torch.full((q, n), -1, dtype=torch.int32, device=device),
           "stat": torch.zeros(q, 8, dtype=torch.int32, device=device),
           "win": torch.full((q, 4), -1, dtype=torch.int32, device=device),
           "hypotheses": torch.zeros(q, dtype=torch.int64, device=device),
           "rms": torch.full((q,), nan, dtype=torch.float64, device=device),
           "num": torch.zeros(4, dtype=torch.int32, device=device)}       # (Q N == 0: the call writes nothing)
    need = relocalize_workspace_bytes(q, n, n_lm, n_stages)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    elif workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("landmarks.relocalize: the workspace must be a contiguous uint8 tensor on %s" % (device,))
    with torch.cuda.device(device):
        engine._check(lib.sgpr_landmark_relocalize(
            engine._ptr(cen), engine._ptr(lab), q, n, engine._ptr(lm_c) if n_lm else None, engine._ptr(lm_l) if n_lm else None,
            engine._ptr(mask) if n_lm else None, n_lm, rad_in.ctypes.data, rad.ctypes.data if n_stages else None, n_stages,
            rad_in.shape[0], float(tau_z), float(tau_edge), float(min_base), float(max_base), int(max_hyp), int(min_inliers),
            float(sep), int(iters), int(min_nodes), engine._ptr(out["poses"]), engine._ptr(out["coarse"]),
            engine._ptr(out["other"]), engine._ptr(out["node_landmark"]), engine._ptr(out["stat"]), engine._ptr(out["win"]),
            engine._ptr(out["hypotheses"]), engine._ptr(out["rms"]), engine._ptr(out["num"]), engine._ptr(workspace),
            workspace.numel(), engine._stream(device)))
    return out


def relocalize(centers, labels, lm, use=None, radius_in=None, radii=(2.0, DEFAULT_RADIUS), tau_z=DEFAULT_TAU_Z, tau_edge=0.5,
               min_base=5.0, max_base=30.0, max_hyp=65536, min_inliers=12, sep=10.0, iters=10, min_nodes=6, workspace=None,
               device=None):
    """Relocalise Q scans in the landmark map `lm` with no prior pose: every pair of nodes of a scan is
    laid on the pairs of landmarks of their labels that are as far apart, the pose with the most nodes on landmarks
    wins, and it is refined through the gates `radii` (every stage an align of that scan).  `inliers_other` is the best
    count among the poses more than `sep` metres from the winner: where it comes close to `inliers` the map repeats
    itself there, and the answer is one of several.  Arguments as relocalize_async.
    -> (poses f64 [Q,4] on the device, NaN for a scan that is not found; info dict of numpy arrays: found bool [Q],
    inliers, inliers_other i32 [Q], coarse, other f64 [Q,4], win i32 [Q,4], hypotheses i64 [Q], matched, live, steps,
    flags i32 [Q], rms f64 [Q], node_landmark i32 [Q,N], num i32 [4] = (scans found, scans truncated, scans without a
    hypothesis, 0))."""
    out = relocalize_async(centers, labels, lm, use=use, radius_in=radius_in, radii=radii, tau_z=tau_z, tau_edge=tau_edge,
                           min_base=min_base, max_base=max_base, max_hyp=max_hyp, min_inliers=min_inliers, sep=sep, iters=iters,
                           min_nodes=min_nodes, workspace=workspace, device=device)
    stat = out["stat"].cpu().numpy()
    return out["poses"], {"found": (stat[:, 5] & RELOC_FOUND) != 0, "inliers": stat[:, 0], "inliers_other": stat[:, 1],
                          "coarse": out["coarse"].cpu().numpy(), "other": out["other"].cpu().numpy(),
                          "win": out["win"].cpu().numpy(), "hypotheses": out["hypotheses"].cpu().numpy(), "matched": stat[:, 2],
                          "live": stat[:, 3], "steps": stat[:, 4], "flags": stat[:, 5], "rms": out["rms"].cpu().numpy(),
                          "node_landmark": out["node_landmark"].cpu().numpy(), "num": out["num"].cpu().numpy()}


def update_workspace_bytes(Q, N, L):
    return int(load_library().sgpr_landmark_update_workspace_bytes(int(Q), int(N), int(L)))


_RECORD = (("center", torch.float64), ("label", torch.int32), ("count", torch.int32), ("first", torch.int32),
           ("sessions", torch.int64), ("spread", torch.float64))


def update_async(centers, labels, poses, assoc, lm, starts=None, session_base=0, node_base=0, radius=None, tau_z=DEFAULT_TAU_Z,
                 max_landmarks=None, workspace=None, device=None):
    """sgpr_landmark_update without reading anything back -> dict of device tensors, asynchronous on the current stream:
    the six record arrays of the updated map with max_landmarks rows (center f64 [.,3], label, count, first i32, sessions
    i64, spread f64), node_landmark i32 [Q,N] (the id in the updated map, -1 = dead or rejected), num i32 [4] = (landmarks
    of the updated map, live nodes, observations, new nodes).  Only the first min(num[0], max_landmarks) records are
    written.  centers f32 [Q,N,3], labels i32 [Q,N], poses [Q,4]: the new scans at their ALIGNED poses; assoc i32 [Q,N]:
    node_landmark of align / align_async against the whole map; lm: the dict of build / update (its six records; the
    inputs are left as they are); starts: the session table of the Q scans; session_base: the number of the first of
    their sessions in the map; node_base: the flat index the map gives their first node (`first` of a new landmark);
    radius, tau_z: the link rule among the new nodes; max_landmarks: default L + Q N, capped at DEFAULT_MAX_LANDMARKS."""
    lib = load_library()
    if device is None:
        device = engine._device_of(centers, labels, poses, lm["center"])
    lab = engine._on(labels, device, torch.int32)
    if lab.dim() != 2:
        raise ValueError("landmarks.update: labels must be [Q, N]")
    q, n = lab.shape
    cen = engine._on(centers, device, torch.float32)
    if cen.numel() != q * n * 3:
        raise ValueError("landmarks.update: centers must be [Q, N, 3]")
    x = engine._on(poses, device, torch.float64)
    if x.numel() != q * 4:
        raise ValueError("landmarks.update: poses must hold one planar pose (c, s, x, y) per scan")
    asc = engine._on(assoc, device, torch.int32)
    if asc.numel() != q * n:
        raise ValueError("landmarks.update: assoc must be [Q, N]")
    old = {k: engine._on(lm[k].view(np.int64) if isinstance(lm[k], np.ndarray) and lm[k].dtype == np.uint64 else lm[k], device, t)
           for k, t in _RECORD}                                     # (a uint64 host mask: its bits)
    n_lm = int(old["label"].numel())
    if old["center"].numel() != 3 * n_lm or any(old[k].numel() != n_lm for k, _ in _RECORD[1:]):
        raise ValueError("landmarks.update: the map must hold center [L,3] and label, count, first, sessions, spread [L]")
    table = engine._session_table(starts)
    rad = _radius_table(radius)
    cap = max(n_lm, min(n_lm + q * n, DEFAULT_MAX_LANDMARKS)) if max_landmarks is None else int(max_landmarks)
    rows = max(cap, 0)
    out = {k: torch.empty((rows, 3) if k == "center" else (rows,), dtype=t, device=device) for k, t in _RECORD}
    out["node_landmark"] = torch.full((q, n), -1, dtype=torch.int32, device=device)
    out["num"] = torch.tensor([n_lm, 0, 0, 0], dtype=torch.int32, device=device)
    if q * n == 0 and rows >= n_lm:                                  # the call writes nothing: the map is what it was
        for k, _ in _RECORD:
            out[k][:n_lm] = old[k].reshape(out[k][:n_lm].shape)
    need = update_workspace_bytes(q, n, n_lm)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    elif workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("landmarks.update: the workspace must be a contiguous uint8 tensor on %s" % (device,))
    with torch.cuda.device(device):
        engine._check(lib.sgpr_landmark_update(
            engine._ptr(cen), engine._ptr(lab), q, n, engine._ptr(x), engine._ptr(asc), *engine._table_args(table),
            int(session_base), int(node_base), rad.ctypes.data, rad.shape[0], float(tau_z),
            *[engine._ptr(old[k]) if n_lm else None for k, _ in _RECORD], n_lm, cap,
            *[engine._ptr(out[k]) if rows else None for k, _ in _RECORD], engine._ptr(out["node_landmark"]),
            engine._ptr(out["num"]), engine._ptr(workspace), workspace.numel(), engine._stream(device)))
    return out


def update(centers, labels, poses, assoc, lm, starts=None, session_base=0, node_base=0, radius=None, tau_z=DEFAULT_TAU_Z,
           max_landmarks=None, workspace=None, device=None):
    """Fold Q aligned scans into the landmark map `lm`: a node that `assoc` puts on a landmark of its
    label becomes one more observation of it (count, centre, sessions and spread move as if it had been a member), the
    nodes with assoc -2 are fused among themselves into new landmarks behind the old ones; old landmarks keep their ids
    and never merge.  Arguments as update_async.
    -> the dict of build - center, label, count, first, sessions, spread trimmed to the landmarks of the updated map,
    node_landmark i32 [Q,N] of the NEW scans, num_landmarks, live_nodes - plus observed and new_nodes; select, align,
    virtual_scans and the next update take it as they take build's, refine takes it together with the new scans (its
    node_landmark is theirs).  If max_landmarks was too small the call is repeated once with the reported count."""
    kw = dict(starts=starts, session_base=session_base, node_base=node_base, radius=radius, tau_z=tau_z, workspace=workspace,
              device=device)
    out = update_async(centers, labels, poses, assoc, lm, max_landmarks=max_landmarks, **kw)
    found, live, seen, new = (int(v) for v in out["num"].tolist())
    if found > out["label"].shape[0]:
        out = update_async(centers, labels, poses, assoc, lm, max_landmarks=found, **kw)
    res = {k: out[k][:found] for k, _ in _RECORD}
    res["node_landmark"] = out["node_landmark"]
    res["num_landmarks"], res["live_nodes"], res["observed"], res["new_nodes"] = found, live, seen, new
    return res


def merge_workspace_bytes(L_a, L_b=0):
    return int(load_library().sgpr_landmark_merge_workspace_bytes(int(L_a), int(L_b)))


def _records_on(lm, device, who):
    """the six record arrays of a map dict on `device`, in the ABI's types -> (dict, L)"""
    rec = {k: engine._on(lm[k].view(np.int64) if isinstance(lm[k], np.ndarray) and lm[k].dtype == np.uint64 else lm[k], device, t)
           for k, t in _RECORD}                                     # (a uint64 host mask: its bits)
    n_lm = int(rec["label"].numel())
    if rec["center"].numel() != 3 * n_lm or any(rec[k].numel() != n_lm for k, _ in _RECORD[1:]):
        raise ValueError("%s: a map must hold center [L,3] and label, count, first, sessions, spread [L]" % who)
    return rec, n_lm


def _keep_on(keep, n_lm, device, who):
    if keep is None:
        return None
    mask = engine._on(torch.as_tensor(keep).reshape(-1) != 0, device, torch.bool).to(torch.uint8)
    if mask.numel() != n_lm:
        raise ValueError("%s: a keep mask must hold one entry per landmark of its map" % who)
    return mask


def merge_async(a, b=None, keep_a=None, keep_b=None, pose=None, session_shift=0, first_base=0, radius=DEFAULT_RADIUS,
                tau_z=None, max_landmarks=None, workspace=None, device=None):
    """sgpr_landmark_merge without reading anything back -> dict of device tensors, asynchronous on the current stream: the
    six record arrays of the merged map with max_landmarks rows (center f64 [.,3], label, count, first i32, sessions i64,
    spread f64), old_to_new i32 [L_a + L_b] (the new id of every input record - A's first, then B's - or -1 of a dropped
    one), num i32 [4] = (landmarks of the merged map, records dropped by a keep mask, kept records dropped as
    ineligible, landmarks fused from more than one record).  Only the first min(num[0], max_landmarks) records are
    written.  a, b: the dicts of build / update / merge (their six records; b None: a is compacted); keep_a, keep_b: masks
    over their landmarks, 0 = drop (persist's keep; None: keep all); pose: planar (c, s, X, Y) that carries b's frame
    into a's (None: b's centres are taken bit for bit); session_shift: b's session bits move up by this many (a bit
    shifted out is lost here - merge raises); first_base: added to b's `first`; radius, tau_z: the link rule among the
    records, as build takes them; max_landmarks: default L_a + L_b, capped at DEFAULT_MAX_LANDMARKS.  workspace: a uint8
    device tensor of at least merge_workspace_bytes(L_a, L_b) to reuse.  The inputs are left as they are."""
    lib = load_library()
    who = "landmarks.merge"
    if device is None:
        device = engine._device_of(a["center"], None if b is None else b["center"])
    rec_a, n_a = _records_on(a, device, who)
    rec_b, n_b = _records_on(b, device, who) if b is not None else (None, 0)
    mask_a = _keep_on(keep_a, n_a, device, who)
    mask_b = _keep_on(keep_b, n_b, device, who) if b is not None else None
    x = None
    if pose is not None:
        x = np.ascontiguousarray(np.asarray(pose.detach().cpu() if isinstance(pose, torch.Tensor) else pose, dtype=np.float64).reshape(-1))
        if x.size != 4:
            raise ValueError("landmarks.merge: pose must be one planar pose (c, s, x, y)")
    rad = _radius_table(radius)
    total = n_a + n_b
    cap = min(total, DEFAULT_MAX_LANDMARKS) if max_landmarks is None else int(max_landmarks)
    rows = max(cap, 0)
    out = {k: torch.empty((rows, 3) if k == "center" else (rows,), dtype=t, device=device) for k, t in _RECORD}
    out["old_to_new"] = torch.full((total,), -1, dtype=torch.int32, device=device)
    out["num"] = torch.zeros(4, dtype=torch.int32, device=device)       # (L_a + L_b == 0: the call writes nothing)
    need = merge_workspace_bytes(n_a, n_b)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    elif workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("landmarks.merge: the workspace must be a contiguous uint8 tensor on %s" % (device,))
    with torch.cuda.device(device):
        engine._check(lib.sgpr_landmark_merge(
            *[engine._ptr(rec_a[k]) if n_a else None for k, _ in _RECORD], engine._ptr(mask_a) if n_a else None, n_a,
            *[engine._ptr(rec_b[k]) if n_b else None for k, _ in _RECORD], engine._ptr(mask_b) if n_b else None, n_b,
            None if x is None else x.ctypes.data, int(session_shift), int(first_base), rad.ctypes.data, rad.shape[0],
            float(DEFAULT_TAU_Z if tau_z is None else tau_z), cap, *[engine._ptr(out[k]) if rows else None for k, _ in _RECORD],
            engine._ptr(out["old_to_new"]), engine._ptr(out["num"]), engine._ptr(workspace), workspace.numel(),
            engine._stream(device)))
    return out


def merge(a, b=None, keep_a=None, keep_b=None, pose=None, session_shift=0, first_base=0, radius=DEFAULT_RADIUS, tau_z=None,
          max_landmarks=None, workspace=None, device=None):
    """Join the landmark maps `a` and `b` on their records alone: what a keep mask drops is gone, records
    of one label within `radius` (and tau_z in height) fuse as if their observations had been fused - inside a, inside b
    and across - and the result is numbered densely, by the lowest input record of every landmark.  Arguments as
    merge_async.  Raises ValueError when session_shift would push a session bit of any record of b out of the 64-bit mask.
    -> the dict of build - center, label, count, first, sessions, spread trimmed to the landmarks of the merged map,
    num_landmarks - plus old_to_new i32 [L_a + L_b] on the device (-1 = dropped; remap carries a node_landmark array
    through it), dropped = (by a keep mask, as ineligible) and fused (landmarks made of more than one record); select,
    align, update, persist, track, relocalize and virtual_scans take it as they take build's.  It holds no node_landmark:
    the node arrays are not read.  If max_landmarks was too small the call is repeated once with the reported count."""
    shift = int(session_shift)
    if b is not None and 0 < shift < 64:
        sess = torch.as_tensor(b["sessions"].view(np.int64) if isinstance(b["sessions"], np.ndarray) and
                               b["sessions"].dtype == np.uint64 else b["sessions"]).to(torch.int64)
        if sess.numel() and bool(((sess >> (64 - shift)) != 0).any()):
            raise ValueError("landmarks.merge: session_shift %d shifts a session bit of b out of the 64-bit mask" % shift)
    kw = dict(keep_a=keep_a, keep_b=keep_b, pose=pose, session_shift=session_shift, first_base=first_base, radius=radius,
              tau_z=tau_z, workspace=workspace, device=device)
    out = merge_async(a, b, max_landmarks=max_landmarks, **kw)
    found, masked, unfit, fused = (int(v) for v in out["num"].tolist())
    if found > out["label"].shape[0]:
        out = merge_async(a, b, max_landmarks=found, **kw)
    res = {k: out[k][:found] for k, _ in _RECORD}
    res["old_to_new"] = out["old_to_new"]
    res["num_landmarks"], res["dropped"], res["fused"] = found, (masked, unfit), fused
    return res


def compact(lm, keep=None, radius=DEFAULT_RADIUS, tau_z=None, max_landmarks=None, workspace=None, device=None):
    """merge with no second map: the landmarks `keep` drops (None: none) and the ineligible ones are removed, duplicates
    within `radius` fuse, the rest keep their order and their bits -> as merge"""
    return merge(lm, None, keep_a=keep, radius=radius, tau_z=tau_z, max_landmarks=max_landmarks, workspace=workspace, device=device)


def remap(node_landmark, old_to_new):
    """Carry a node_landmark array (of build, align, update, track or relocalize; any shape) through merge's old_to_new
    table: an id >= 0 becomes its new id, or -2 - "the map does not explain this node" - where its landmark was dropped;
    -1 and -2 stay.  For the nodes of map b the ids are first raised by L_a by the caller.  -> int32, a tensor on
    node_landmark's device when that is a tensor, else a numpy array."""
    if isinstance(node_landmark, torch.Tensor):
        node = node_landmark.to(torch.int64)
        table = torch.as_tensor(old_to_new).to(device=node.device, dtype=torch.int64).reshape(-1)
        if table.numel() == 0:
            return torch.where(node >= 0, torch.full_like(node, -2), node).to(torch.int32)
        new = table[node.clamp(0, table.numel() - 1)]
        new = torch.where(new >= 0, new, torch.full_like(new, -2))
        return torch.where((node >= 0) & (node < table.numel()), new, torch.where(node >= 0, torch.full_like(node, -2), node)).to(torch.int32)
    node = np.asarray(node_landmark).astype(np.int64)
    table = np.asarray(old_to_new.cpu() if isinstance(old_to_new, torch.Tensor) else old_to_new).astype(np.int64).reshape(-1)
    out = np.where(node >= 0, -2, node)
    inside = (node >= 0) & (node < table.size)
    new = table[node[inside]]
    out[inside] = np.where(new >= 0, new, -2)
    return out.astype(np.int32)


def persist_workspace_bytes(Q, N, L):
    return int(load_library().sgpr_landmark_persist_workspace_bytes(int(Q), int(N), int(L)))


def persist_async(centers, labels, poses, assoc, lm, use=None, radius=None, max_range=50.0, margin=2.0, min_expected=5,
                  max_seen_ratio=0.3, workspace=None, device=None):
    """sgpr_landmark_persist without reading anything back -> dict of device tensors, asynchronous on the current stream:
    expected, seen i32 [L] (the scans that should have seen the landmark / that did), keep u8 [L] (0 = retired),
    scan_stat i32 [Q,4] = (landmarks the scan should have seen, landmarks it saw, live nodes, flags: ALIGN_NONFINITE),
    view f64 [Q] (the view range of the scan, metres), num i32 [4] = (retired, eligible landmarks with expected >=
    min_expected, eligible landmarks, scans with a view).  centers f32 [Q,N,3], labels i32 [Q,N], poses [Q,4]: the scans
    of ONE drive at their aligned poses; assoc i32 [Q,N]: node_landmark of align (iters=0, every landmark) or of update; lm:
    the dict of build / update ("center", "label"); use: a mask over the landmarks that take part (None: all); radius:
    the table that says which labels take part (a label of radius 0 does not); max_range: the sensor range, margin: what
    is taken off a scan's range, both metres; a landmark is retired with expected >= min_expected and seen <
    max_seen_ratio * expected.  workspace: a uint8 device tensor of at least persist_workspace_bytes(Q, N, L) to reuse."""
    lib = load_library()
    if device is None:
        device = engine._device_of(centers, labels, poses, lm["center"])
    lab = engine._on(labels, device, torch.int32)
    if lab.dim() != 2:
        raise ValueError("landmarks.persist: labels must be [Q, N]")
    q, n = lab.shape
    cen = engine._on(centers, device, torch.float32)
    if cen.numel() != q * n * 3:
        raise ValueError("landmarks.persist: centers must be [Q, N, 3]")
    x = engine._on(poses, device, torch.float64)
    if x.numel() != q * 4:
        raise ValueError("landmarks.persist: poses must hold one planar pose (c, s, x, y) per scan")
    asc = engine._on(assoc, device, torch.int32)
    if asc.numel() != q * n:
        raise ValueError("landmarks.persist: assoc must be [Q, N]")
    lm_c = engine._on(lm["center"], device, torch.float64)
    lm_l = engine._on(lm["label"], device, torch.int32)
    n_lm = int(lm_l.numel())
    if lm_c.numel() != 3 * n_lm:
        raise ValueError("landmarks.persist: the map must hold center [L,3] and label [L]")
    mask = None
    if use is not None:
        mask = engine._on(torch.as_tensor(use).reshape(-1) != 0, device, torch.bool).to(torch.uint8)
        if mask.numel() != n_lm:
            raise ValueError("landmarks.persist: use must hold one entry per landmark")
    rad = _radius_table(radius)
    out = {"expected": torch.zeros(n_lm, dtype=torch.int32, device=device),
           "seen": torch.zeros(n_lm, dtype=torch.int32, device=device),
           "keep": torch.ones(n_lm, dtype=torch.uint8, device=device),
           "scan_stat": torch.zeros(q, 4, dtype=torch.int32, device=device),
           "view": torch.zeros(q, dtype=torch.float64, device=device),
           "num": torch.zeros(4, dtype=torch.int32, device=device)}       # (Q N == 0: the call writes nothing)
    need = persist_workspace_bytes(q, n, n_lm)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    elif workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("landmarks.persist: the workspace must be a contiguous uint8 tensor on %s" % (device,))
    with torch.cuda.device(device):
        engine._check(lib.sgpr_landmark_persist(
            engine._ptr(cen), engine._ptr(lab), q, n, engine._ptr(x), engine._ptr(asc), engine._ptr(lm_c) if n_lm else None,
            engine._ptr(lm_l) if n_lm else None, engine._ptr(mask) if n_lm else None, n_lm, rad.ctypes.data, rad.shape[0],
            float(max_range), float(margin), int(min_expected), float(max_seen_ratio),
            engine._ptr(out["expected"]) if n_lm else None, engine._ptr(out["seen"]) if n_lm else None,
            engine._ptr(out["keep"]) if n_lm else None, engine._ptr(out["scan_stat"]), engine._ptr(out["view"]),
            engine._ptr(out["num"]), engine._ptr(workspace), workspace.numel(), engine._stream(device)))
    return out


def persist(centers, labels, poses, assoc, lm, use=None, radius=None, max_range=50.0, margin=2.0, min_expected=5,
            max_seen_ratio=0.3, prior=None, workspace=None, device=None):
    """What one drive should have seen of the landmark map `lm` and what it saw.  A scan sees what lies
    within the range of its farthest live node, capped by max_range, less margin; a landmark is EXPECTED by every scan
    that has it in view or observes it, SEEN by every scan with a node on it (assoc), and retired - keep 0 - when the
    drive expected it at least min_expected times and saw it in less than max_seen_ratio of those.  There is no
    occlusion model.  Arguments as persist_async; prior: (expected, seen) of earlier drives, added into the tallies
    returned - lifetime tallies; keep stays THIS drive's decision.
    -> dict: expected, seen i32 [L] and keep bool [L] on the device (select(lm, keep=...) takes it); numpy arrays
    scan_expected, scan_seen, scan_live, flags i32 [Q], view f64 [Q], num i32 [4] = (retired, eligible landmarks with expected >= min_expected,
    eligible landmarks, scans with a view)."""
    out = persist_async(centers, labels, poses, assoc, lm, use=use, radius=radius, max_range=max_range, margin=margin,
                        min_expected=min_expected, max_seen_ratio=max_seen_ratio, workspace=workspace, device=device)
    expected, seen = out["expected"], out["seen"]
    if prior is not None:
        dev = expected.device
        p_exp, p_seen = (engine._on(torch.as_tensor(t).reshape(-1), dev, torch.int32) for t in prior)
        if p_exp.numel() > expected.numel() or p_seen.numel() != p_exp.numel():
            raise ValueError("landmarks.persist: prior holds (expected, seen) of at most the map's landmarks")
        expected, seen = expected.clone(), seen.clone()              # (a map that grew: the new landmarks have no prior)
        expected[:p_exp.numel()] += p_exp
        seen[:p_seen.numel()] += p_seen
    stat = out["scan_stat"].cpu().numpy()
    return {"expected": expected, "seen": seen, "keep": out["keep"] != 0, "scan_expected": stat[:, 0], "scan_seen": stat[:, 1],
            "scan_live": stat[:, 2], "flags": stat[:, 3], "view": out["view"].cpu().numpy(),
            "num": out["num"].cpu().numpy()}


def virtual_scans(lm, poses, sensor_range=50.0, node_num=100, keep=None):
    """What a scan at each of `poses` [Q,4] (planar, sensor into map) would hold if it saw the landmarks themselves:
    the kept landmarks (keep: a mask as select makes it; None: all) within sensor_range of the pose (planar), in the
    sensor frame - inverse(pose) applied to the centre, z unchanged - the nearest node_num of them (ties to the lower
    landmark id), listed label-ascending (stable), padded with centre 0 / label -1: the layout synth.world_sequence
    makes and verify_pairs / embed read.  -> (centers f32 [Q,node_num,3], labels i32 [Q,node_num]) on lm's device."""
    center = torch.as_tensor(lm["center"])
    dev = center.device
    center = center.to(torch.float64).reshape(-1, 3)
    label = torch.as_tensor(lm["label"]).to(device=dev, dtype=torch.int64).reshape(-1)
    if keep is not None:
        idx = torch.nonzero(torch.as_tensor(keep).to(device=dev, dtype=torch.bool).reshape(-1)).reshape(-1)
        center, label = center[idx], label[idx]                 # (ascending: ties still go to the lower id)
    X = engine._on(poses, dev, torch.float64).reshape(-1, 4)
    q, n_lm, nn = X.shape[0], center.shape[0], int(node_num)
    out_c = torch.zeros(q, nn, 3, dtype=torch.float32, device=dev)
    out_l = torch.full((q, nn), -1, dtype=torch.int32, device=dev)
    if q == 0 or n_lm == 0 or nn == 0:
        return out_c, out_l
    k = min(nn, n_lm)
    step = max(1, _CHUNK_BYTES // (8 * n_lm))
    r2 = float(sensor_range) * float(sensor_range)
    big = 1 << 20
    for lo in range(0, q, step):
        P = X[lo:lo + step]
        dx = center[None, :, 0] - P[:, None, 2]
        dy = center[None, :, 1] - P[:, None, 3]
        d2 = dx * dx + dy * dy
        d2 = torch.where(d2 <= r2, d2, torch.full_like(d2, float("inf")))
        # nearest first, ties to the lower id: a stable sort of the distances
        dist, near = torch.sort(d2, dim=1, stable=True)
        dist, near = dist[:, :k], near[:, :k]
        seen = torch.isfinite(dist)
        lab = torch.where(seen, label[near], torch.full_like(near, big))
        order = torch.argsort(lab, dim=1, stable=True)          # label-ascending, unseen last
        near, seen, lab = near.gather(1, order), seen.gather(1, order), lab.gather(1, order)
        ex, ey = dx.gather(1, near), dy.gather(1, near)
        c, s = P[:, None, 0], P[:, None, 1]
        pts = torch.stack((c * ex + s * ey, c * ey - s * ex, center[:, 2][near]), dim=-1)     # R^T (centre - t)
        out_c[lo:lo + step, :k] = torch.where(seen[..., None], pts, torch.zeros_like(pts)).to(torch.float32)
        out_l[lo:lo + step, :k] = torch.where(seen, lab, torch.full_like(lab, -1)).to(torch.int32)
    return out_c, out_l

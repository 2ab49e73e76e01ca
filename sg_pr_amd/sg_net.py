"""`SG` / `SGTrainer` with the reference's API (sg_net.py:18-138, 141-206, 241-310,
434-525) backed by the MI355X HIP engine.

Only inference is built here (training lives in sg_pr_amd.train): the model
must be in eval mode - BatchNorm running statistics are folded into the kernels'
weights.  There is no CPU fallback.
"""
import os
import warnings
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import engine as _engine
from .layers_batch import AttentionModule, TenorNetworkModule
from .utils import process_pair, load_paires, read_graph, pose_distance  # noqa: F401  (reference: `from utils import *`)


def _planar(p):
    """poses as optimize_map and localize take them - KITTI rows [M,12] or planar [M,4] - as planar float64 [M,4] on the host"""
    from . import metrics
    p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
    p = p.reshape(p.shape[0], -1)
    return np.asarray(p, dtype=np.float64) if p.shape[1] == 4 else metrics.planar_odometry(p)


class SG(torch.nn.Module):
    """Pair scorer with the reference's constructor, parameter names and forward contract.

    `state_dict()` has exactly the reference's 50 keys, so any shipped checkpoint
    loads strictly.  `forward(data)` returns `(score[B], att1[B,N,1], att2[B,N,1])`.
    """

    def __init__(self, args, number_of_labels):
        super(SG, self).__init__()
        self.args = args
        self.number_labels = number_of_labels
        self.setup_layers()
        self._engine = None
        self._engine_key = None

    def calculate_bottleneck_features(self):
        self.feature_count = self.args.tensor_neurons

    def setup_layers(self):
        a = self.args
        self.calculate_bottleneck_features()
        self.attention = AttentionModule(a)
        self.tensor_network = TenorNetworkModule(a)
        self.fully_connected_first = torch.nn.Linear(self.feature_count, a.bottle_neck_neurons)
        self.scoring_layer = torch.nn.Linear(a.bottle_neck_neurons, 1)

        def block2d(cin, cout):
            return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, bias=False), nn.BatchNorm2d(cout),
                                 nn.LeakyReLU(negative_slope=0.2))

        self.dgcnn_s_conv1 = block2d(3 * 2, a.filters_1)
        self.dgcnn_f_conv1 = block2d(self.number_labels * 2, a.filters_1)
        self.dgcnn_s_conv2 = block2d(a.filters_1 * 2, a.filters_2)
        self.dgcnn_f_conv2 = block2d(a.filters_1 * 2, a.filters_2)
        self.dgcnn_s_conv3 = block2d(a.filters_2 * 2, a.filters_3)
        self.dgcnn_f_conv3 = block2d(a.filters_2 * 2, a.filters_3)
        self.dgcnn_conv_end = nn.Sequential(nn.Conv1d(a.filters_3 * 2, a.filters_3, kernel_size=1, bias=False),
                                            nn.BatchNorm1d(a.filters_3), nn.LeakyReLU(negative_slope=0.2))

    # ------------------------------------------------------------------ engine plumbing
    @property
    def module(self):
        """The reference wraps the model in DataParallel; `.module` keeps such callers working."""
        return self

    def _device_index(self):
        return int(getattr(self.args, "gpu", 0))

    def engine(self):
        """The packed-weights HIP handle for the current parameters (rebuilt if they change)."""
        if self.training:
            raise RuntimeError("sg_pr_amd.SG only runs in eval mode (BatchNorm statistics are folded into the "
                               "HIP kernels); call model.eval() - training is not part of this engine")
        key = tuple(t._version for t in list(self.parameters()) + list(self.buffers())) + (self._device_index(),)
        if self._engine is None or key != self._engine_key:
            if self._engine is not None:
                self._engine.close()
            self._engine = _engine.Engine(self.state_dict(), _engine.dims_from_args(self.args, self.number_labels),
                                          device=self._device_index())
            self._engine_key = key
        return self._engine

    def _apply(self, fn, *a, **k):
        # .cuda()/.to() of the torch parameters does not move the packed copy: drop it
        self._engine_key = None
        return super()._apply(fn, *a, **k)

    # ------------------------------------------------------------------ reference API
    def dgcnn_conv_pass(self, x):
        """sg_net.py:79-110 - x [B, 3+L, N] -> node embeddings [B, N, filters_3]."""
        _, _, emb = self.engine().embed_dense(x, int(self.args.K), want_emb=True)
        return emb

    def forward(self, data):
        """sg_net.py:112-138 - data["features_1"/"features_2"]: [B, 3+L, N]."""
        score, att1, att2 = self.engine().forward_dense(data["features_1"], data["features_2"], int(self.args.K))
        return score, att1.unsqueeze(-1), att2.unsqueeze(-1)

    # ------------------------------------------------------------------ packed fast paths (no one-hot tensors)
    def embed(self, centers, labels, want_att=False, want_emb=False, node_cap=None, order=None):
        """Packed graphs (centers [G,N,3], labels [G,N], -1 = pad) -> pooled [G, filters_3] (+att, +emb).
        node_cap: promise on the slots processed per graph; order: launch order, largest graphs first
        (engine.Engine.size_order gives both).  Host arrays get them computed automatically; device tensors run
        without unless given (computing them would synchronise).
        Contract: the launch is asynchronous and does NOT report bad labels / a broken node_cap promise by itself
        (affected graphs get all-zero semantic rows / a NaN pooled vector); call `engine().check_status()` once the
        results are needed - the evaluation entry points (forward_packed, eval_batch_pair, eval_batch.score_pair_list,
        graph_store.evaluate_all_pairs) do."""
        eng = self.engine()
        from .allpairs import RaggedGraphs
        if isinstance(centers, RaggedGraphs):
            # the ragged store (sgpr_embed_ragged): its offsets live on the host, so the launch plan costs no synchronisation
            rag = centers
            if node_cap is None and order is None and len(rag):
                order, node_cap = eng.ragged_order(rag.offsets, rag.node_num, int(self.args.K))
            return eng.embed_ragged(rag.centers, rag.labels, rag.offsets - rag.offsets[0], rag.node_num, int(self.args.K),
                                    want_att=want_att, want_emb=want_emb, node_cap=node_cap or 0, order=order)
        if node_cap is None and order is None:
            if not (isinstance(labels, torch.Tensor) and labels.is_cuda) and len(labels):
                order, node_cap = eng.size_order(centers, labels, int(self.args.K))
        return eng.embed(centers, labels, int(self.args.K), want_att=want_att, want_emb=want_emb,
                         node_cap=node_cap or 0, order=order)

    GROUPED_MIN_PAIRS = 2048     # below this the one-wave-per-pair kernel's single launch wins

    def score_pooled(self, pooled_1, pooled_2, idx_1=None, idx_2=None, grouped=None):
        """NTN + head on pooled vectors (optionally gathered through index lists).  A list of GROUPED_MIN_PAIRS pairs
        or more over shared graphs - the reference's evaluation loop, eval_batch.py:30-36 - is grouped by row graph
        once on the host and scored by sgpr_score_pair_list (matrix cores, bilinear form hoisted per distinct row
        graph); shorter lists and un-indexed sides take sgpr_score_pairs (one wave per pair, exact fp32).
        grouped: True / False picks the kernel regardless of the length (a caller that holds one SHARD of a list decides
        on the whole list's length, so that a pair's bits do not depend on how the list was split); None = by length."""
        eng = self.engine()
        if grouped is None:
            grouped = idx_1 is not None and idx_2 is not None and len(idx_1) >= self.GROUPED_MIN_PAIRS
        if self.engine().any_shape:          # (an architecture beyond the built shape: the grouped kernel is not built for it)
            grouped = False
        if grouped and idx_1 is not None and idx_2 is not None and len(idx_1) > 0:
            i1 = idx_1.cpu().numpy() if isinstance(idx_1, torch.Tensor) else np.asarray(idx_1)
            i2 = idx_2.cpu().numpy() if isinstance(idx_2, torch.Tensor) else np.asarray(idx_2)
            plan = eng.pair_plan(i1, i2, pooled_1.shape[0], pooled_2.shape[0])
            return eng.score_pair_list(pooled_1, pooled_2, plan)
        return eng.score_pairs(pooled_1, pooled_2, idx_1, idx_2)

    def score_all_pairs(self, pooled_rows, pooled_cols, out=None):
        return self.engine().score_all_pairs(pooled_rows, pooled_cols, out=out)

    def loop_closures(self, pooled_rows, pooled_cols, k=1, window=-1, row0=0, causal=False, row_self=None, seq_len=1,
                      seq_reverse="both", distinct=None, seq_slopes=None, row_sessions=None, col_sessions=None):
        """The k best columns per row of pooled_rows x pooled_cols without forming the matrix (engine.Engine.score_topk)
        -> (values f32 [R,k], indices i32 [R,k]) on the device.  seq_len > 1: rows and columns are consecutive scans and
        the lists rank the sequence-matched score (engine.Engine.score_seq_topk; seq_reverse False / True / "both")
        -> (values, indices, dirs u8 [R,k]).  distinct=rho (0..1024): rows and columns are consecutive scans and the
        lists hold distinct places - the k best PEAKS of the ranked score, a peak being the first column, by (value
        descending, column ascending), among the qualifying columns at most rho away (engine.Engine.score_peak_topk,
        DESIGN.md §20; k up to 4096, choose rho <= window); seq_len still chooses the score and the shape of the
        result.  distinct=None: the plain lists.  seq_slopes (with seq_len > 1; e.g. ("1", "1/2", "2/3", "3/2", "2")): the
        score is the best mean over a set of paths of these slopes - a revisit driven at another speed
        (engine.seq_paths, engine.Engine.score_path_topk) -> (values, indices, codes u8 [R,k]: direction
        bit | path << 1); it composes with distinct.  seq_slopes=None: the unit diagonal, exactly as before.
        row_sessions / col_sessions (the first row / column of every session of a stacked multi-session map; either may
        be None: one session): sums and the window stop at session boundaries (engine.Engine.score_session_topk,
        DESIGN.md §22) -> (values, indices, codes), for every seq_len; not with distinct.  Both None: exactly as before."""
        if row_sessions is not None or col_sessions is not None:
            if distinct is not None:
                raise ValueError("loop_closures: distinct is not available with session tables")
            if seq_slopes is not None and int(seq_len) == 1:
                raise ValueError("loop_closures: seq_slopes needs seq_len > 1")
            paths = None if seq_slopes is None else _engine.seq_paths(int(seq_len), seq_slopes)
            return self.engine().score_session_topk(pooled_rows, pooled_cols, int(seq_len), paths,
                                                    row_sessions=row_sessions, col_sessions=col_sessions, k=k,
                                                    window=window, row0=row0, causal=causal, row_self=row_self,
                                                    reverse=seq_reverse)
        if seq_slopes is not None:
            if int(seq_len) == 1:
                raise ValueError("loop_closures: seq_slopes needs seq_len > 1")
            return self.engine().score_path_topk(pooled_rows, pooled_cols, int(seq_len),
                                                 _engine.seq_paths(int(seq_len), seq_slopes), k=k,
                                                 radius=0 if distinct is None else int(distinct), window=window, row0=row0,
                                                 causal=causal, row_self=row_self, reverse=seq_reverse)
        if distinct is not None:
            out = self.engine().score_peak_topk(pooled_rows, pooled_cols, int(distinct), seq_len=int(seq_len), k=k,
                                                window=window, row0=row0, causal=causal, row_self=row_self,
                                                reverse=seq_reverse if int(seq_len) != 1 else False)
            return out if int(seq_len) != 1 else out[:2]
        if int(seq_len) != 1:
            return self.engine().score_seq_topk(pooled_rows, pooled_cols, int(seq_len), k=k, window=window, row0=row0,
                                                causal=causal, row_self=row_self, reverse=seq_reverse)
        return self.engine().score_topk(pooled_rows, pooled_cols, k=k, window=window, row0=row0, causal=causal,
                                        row_self=row_self)

    def verify_closures(self, centers, labels, indices, values=None, min_inliers=None, col_centers=None, col_labels=None,
                        **tolerances):
        """Geometric verification of candidate lists (engine.verify_pairs): indices [R,k] as every
        loop_closures* call returns them - row r lists column graphs for row graph r of (centers [R,N,3], labels [R,N]);
        the columns index (col_centers, col_labels), by default the row graphs themselves.  A -1 padding slot is
        skipped: its fields are zero and its flags VERIFY_INVALID_INDEX.
        -> dict of device tensors: every field of engine.verify_pairs shaped [R,k,...]; order i64 [R,k] = the slots of
        each row re-ranked by (refined inliers descending, score descending, column ascending; padding last; values
        None: all scores equal) and indices_ranked = the columns in that order; with min_inliers also accept bool
        [R,k] = inliers_refined >= min_inliers (never a padding slot).  tolerances: tau_edge, tau_inlier, tau_z,
        min_base, max_hyp."""
        dev = self.engine().device
        idx = torch.as_tensor(indices).to(device=dev, dtype=torch.int32)
        if idx.dim() != 2:
            raise ValueError("verify_closures: indices must be [R, k]")
        r, k = idx.shape
        rows = torch.arange(r, dtype=torch.int32, device=dev).repeat_interleave(k)
        cc, cl = (centers, labels) if col_centers is None else (col_centers, col_labels)
        flat = _engine.verify_pairs(centers, labels, cc, cl, rows, idx.reshape(-1), device=dev, **tolerances)
        out = {name: t.reshape((r, k) + tuple(t.shape[1:])) for name, t in flat.items()}
        valid = idx >= 0
        order = torch.argsort(torch.where(valid, idx, torch.full_like(idx, 0x7fffffff)), dim=1, stable=True)
        if values is not None:
            score = torch.as_tensor(values).to(device=dev, dtype=torch.float32).reshape(r, k)
            order = order.gather(1, torch.argsort(-score.gather(1, order), dim=1, stable=True))
        inl = torch.where(valid, out["inliers_refined"], torch.full_like(idx, -1))
        order = order.gather(1, torch.argsort(-inl.gather(1, order), dim=1, stable=True))
        out["order"] = order
        out["indices_ranked"] = idx.gather(1, order)
        if min_inliers is not None:
            out["accept"] = valid & (out["inliers_refined"] >= int(min_inliers))
        return out

    def consistent_closures(self, verified, rows, cols, row_poses, col_poses=None, row_sessions=None, col_sessions=None,
                            max_trans=1.0, max_yaw=0.06, lever_gain=0.04, min_clique=3):
        """Pairwise-consistent closures (engine.closure_consistency + engine.consistent_set): of the
        verified closures, per pair of sessions, a largest-by-greedy set whose members agree with one another through the
        odometry - going out over one closure and back over another returns to the start within max_trans + lever_gain x
        (distance between the two row scans) metres and max_yaw radians.
        verified: the dict of verify_closures / engine.verify_pairs ("refined", "flags", and "accept" when it was made
        with min_inliers); rows / cols: the row and column scan of every closure, same shape as the records (at most
        engine.CONSISTENCY_MAX_CLOSURES in all); row_poses / col_poses: KITTI 3x4 pose rows [M,12] (metrics.planar_odometry
        makes them planar) or planar poses [M,4]; col_poses None: the row poses.  row_sessions / col_sessions: the first
        scan of every session of a stacked map (None: one session); closures are only compared within one (row session,
        column session) group.  A closure is void - never selected, consistent with nothing - if its flags carry
        INVALID_INDEX, NO_HYPOTHESIS or NONFINITE or it is not accepted; a group whose set is smaller than min_clique
        accepts nothing.
        -> dict of device tensors shaped like rows: accept bool, rank i32 (the order chosen within the group, -1 = not),
        degree i32 (closures of its group it agrees with); group_size i32 [row sessions x column sessions]."""
        import math
        from . import metrics
        dev = self.engine().device
        r = torch.as_tensor(rows).to(device=dev, dtype=torch.int64)
        shape = tuple(r.shape)
        r = r.reshape(-1)
        c = torch.as_tensor(cols).to(device=dev, dtype=torch.int64).reshape(-1)
        flags = torch.as_tensor(verified["flags"]).to(device=dev, dtype=torch.int64).reshape(-1)
        refined = torch.as_tensor(verified["refined"]).to(device=dev, dtype=torch.float64).reshape(-1, 4)
        if c.numel() != r.numel() or flags.numel() != r.numel() or refined.shape[0] != r.numel():
            raise ValueError("consistent_closures: rows, cols and the verified records must have the same shape")

        def planar(p):
            p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
            p = p.reshape(p.shape[0], -1)
            return torch.as_tensor(np.asarray(p, dtype=np.float64) if p.shape[1] == 4 else metrics.planar_odometry(p),
                                   device=dev)

        def starts(t):
            t = [0] if t is None else (t.cpu().numpy() if isinstance(t, torch.Tensor) else t)
            return torch.as_tensor(np.asarray(t, dtype=np.int64).reshape(-1), device=dev)

        xr = planar(row_poses)
        xc = xr if col_poses is None else planar(col_poses)
        rs, cs = starts(row_sessions), starts(col_sessions)
        n_groups = int(rs.numel() * cs.numel())
        void = (flags & (_engine.VERIFY_INVALID_INDEX | _engine.VERIFY_NO_HYPOTHESIS | _engine.VERIFY_NONFINITE)) != 0
        if "accept" in verified:
            void |= ~torch.as_tensor(verified["accept"]).to(device=dev, dtype=torch.bool).reshape(-1)
        group = (torch.searchsorted(rs, r, right=True) - 1) * cs.numel() + (torch.searchsorted(cs, c, right=True) - 1)
        group = torch.where(void | (r < 0) | (c < 0), torch.full_like(group, -1), group)
        adj, degree, members = _engine.closure_consistency(r, c, refined, xr, xc, group, n_groups, max_trans,
                                                           math.cos(float(max_yaw)), lever_gain, device=dev)
        rank, size = _engine.consistent_set(adj, members, n_groups, device=dev)
        big = size[members.clamp(min=0).to(torch.int64)] >= int(min_clique)
        return {"accept": ((rank >= 0) & big).reshape(shape), "rank": rank.reshape(shape),
                "degree": degree.reshape(shape), "group_size": size}

    def optimize_map(self, consistent, verified, rows, cols, poses, sessions=None, row_poses=None, row_sessions=None,
                     weight=None, **solver):
        """One map in one frame (posegraph.optimize): the closures consistent_closures accepted become the
        loop edges of a planar pose graph over the odometry of the map, and a two-stage linear solve spreads the drift
        over the loops and places every session that a closure ties to the first one.
        consistent: the dict of consistent_closures (its "accept") or a bool mask shaped like rows; verified: the dict of
        verify_closures / engine.verify_pairs ("refined"); rows / cols: the row and column scan of every closure.  poses
        / sessions: the column scans' poses (KITTI rows [M,12] or planar [M,4]) and session table.  row_poses None: the
        rows index the same map; otherwise the row scans are a separate set, joined to the map behind the column scans
        as extra sessions (row_sessions: its own session table, None = one).  The first scan of the first session is
        fixed.  solver: weight, w_odo, w_clo, max_iters, rel_tol of posegraph.optimize.
        -> (planar poses f64 [M (+ MR), 4] device tensor in the frame of the first session, info dict with
        "session_starts" of the stacked map added)."""
        from . import posegraph
        dev = self.engine().device

        def table(t):
            t = [0] if t is None else (t.cpu().numpy() if isinstance(t, torch.Tensor) else t)
            return np.asarray(t, dtype=np.int64).reshape(-1)

        X, starts = _planar(poses), table(sessions)
        r = torch.as_tensor(rows).to(device=dev, dtype=torch.int64).reshape(-1)
        c = torch.as_tensor(cols).to(device=dev, dtype=torch.int64).reshape(-1)
        if row_poses is not None:
            r = torch.where(r >= 0, r + X.shape[0], r)
            starts = np.concatenate((starts, table(row_sessions) + X.shape[0]))
            X = np.concatenate((X, _planar(row_poses)))
        acc = consistent["accept"] if isinstance(consistent, dict) else consistent
        acc = torch.as_tensor(acc).to(device=dev, dtype=torch.bool).reshape(-1)
        refined = torch.as_tensor(verified["refined"]).to(device=dev, dtype=torch.float64).reshape(-1, 4)
        if not (acc.numel() == r.numel() == c.numel() == refined.shape[0]):
            raise ValueError("optimize_map: the selection, the verified records, rows and cols must have the same shape")
        if weight is not None:
            weight = torch.as_tensor(weight).to(device=dev, dtype=torch.float64).reshape(-1)[acc]
        out, info = posegraph.optimize(X, r[acc].to(torch.int32), c[acc].to(torch.int32), refined[acc], starts=starts,
                                       weight=weight, device=dev, **solver)
        info["session_starts"] = starts.astype(np.int32)
        return out, info

    def localize(self, verified, cols, map_poses, query_poses=None, query_sessions=None, seq_len=1, min_support=3,
                 max_trans=1.0, max_yaw=0.1):
        """Where is every query scan in the map (localize.localize): every verified candidate of the last
        seq_len scans of a query's session, carried forward by the query drive's own odometry, is a hypothesis of the
        query's pose in the map; the answer is the mean of the largest set of hypotheses that agrees with one of them
        within max_trans metres and max_yaw radians, accepted when that set has min_support members.
        verified: the dict of verify_closures ("refined", "flags", and "accept" when it was made with min_inliers) with
        the queries as rows, shaped [Q,k]; cols [Q,k]: the candidate map scans (-1 = padding).  map_poses: the poses of
        the map scans in the map frame - KITTI rows [M,12] (metrics.planar_odometry makes them planar) or planar [M,4],
        e.g. what optimize_map returned.  query_poses: the odometry of the query drive in any frame of its own (needed
        for seq_len > 1), query_sessions its session table (None: one session).  A candidate is void if its flags carry
        INVALID_INDEX, NO_HYPOTHESIS or NONFINITE or it is not accepted.
        -> dict of device tensors: pose f64 [Q,4] (c, s, x, y; NaN without a live hypothesis), support, live, winner,
        flags i32 [Q], spread f64 [Q], accept bool [Q]."""
        from . import localize as _localize
        dev = self.engine().device
        c = torch.as_tensor(cols).to(device=dev, dtype=torch.int32)
        if c.dim() != 2:
            raise ValueError("localize: cols must be [Q, k]")
        flags = torch.as_tensor(verified["flags"]).to(device=dev, dtype=torch.int64).reshape(c.shape)
        refined = torch.as_tensor(verified["refined"]).to(device=dev, dtype=torch.float64).reshape(tuple(c.shape) + (4,))
        void = (flags & (_engine.VERIFY_INVALID_INDEX | _engine.VERIFY_NO_HYPOTHESIS | _engine.VERIFY_NONFINITE)) != 0
        if "accept" in verified:
            void |= ~torch.as_tensor(verified["accept"]).to(device=dev, dtype=torch.bool).reshape(c.shape)
        if int(seq_len) > 1 and query_poses is None:
            raise ValueError("localize: seq_len > 1 needs the query drive's odometry (query_poses)")
        odo = None if query_poses is None else _planar(query_poses)
        return _localize.localize(_planar(map_poses), c, refined, accept=~void, odo=odo, starts=query_sessions,
                                  seq_len=int(seq_len), max_trans=max_trans, max_yaw=max_yaw, device=dev,
                                  min_support=int(min_support))

    def landmark_map(self, centers, labels, poses, sessions=None, **kw):
        """The semantic landmark map (landmarks.build): the nodes of every scan of the map, put into the
        map frame by the scan's pose and fused - nodes of one label within a radius of one another are one landmark.
        centers [M,N,3], labels [M,N]: the packed node arrays of the map scans; poses: KITTI rows [M,12] or planar
        [M,4], e.g. what optimize_map returned; sessions: the session table of the scans (None: one session).
        kw: radius, tau_z, max_landmarks, workspace of landmarks.build.
        -> its dict: center, label, count, first, sessions, spread per landmark, node_landmark [M,N], num_landmarks,
        live_nodes."""
        from . import landmarks as _landmarks
        x = poses if isinstance(poses, torch.Tensor) and poses.dim() == 2 and poses.shape[1] == 4 else _planar(poses)
        return _landmarks.build(centers, labels, x, starts=sessions, device=self.engine().device, **kw)

    def refine_map(self, centers, labels, poses, sessions=None, rounds=2, iters=10, min_count=2, min_sessions=1,
                   fixed=None, min_nodes=6, **landmark_kw):
        """Refine the poses of a map on its own landmarks (landmarks.refine): `rounds` times, the landmark
        map is built on the current poses (landmark_map), the landmarks with at least min_count observations from at
        least min_sessions sessions are selected (landmarks.select), and `iters` alternations of centre means and
        closed-form pose fits move every scan onto them; a final landmark map is built on the result.  Re-associating
        between the rounds lets landmarks that drift had merged or split come right.
        centers [M,N,3], labels [M,N]; poses: KITTI rows [M,12] or planar [M,4], e.g. what optimize_map returned;
        sessions: the session table of the scans (None: one session); fixed: a mask over the scans that keep their pose
        (None: the first scan of the first session); landmark_kw: radius, tau_z of landmarks.build.
        -> (planar poses f64 [M,4] device tensor, the dict of landmark_map on them, [numpy cost array per round])."""
        from . import landmarks as _landmarks
        dev = self.engine().device
        x = poses if isinstance(poses, torch.Tensor) and poses.dim() == 2 and poses.shape[1] == 4 else _planar(poses)
        x = _engine._on(x, dev, torch.float64)
        if fixed is None:
            fixed = torch.zeros(x.shape[0], dtype=torch.bool, device=dev)
            fixed[:1] = True
        costs = []
        for _ in range(int(rounds)):
            lm = _landmarks.build(centers, labels, x, starts=sessions, device=dev, **landmark_kw)
            use = _landmarks.select(lm, min_count=min_count, min_sessions=min_sessions)
            x, info = _landmarks.refine(centers, labels, x, lm, use=use, fixed=fixed, iters=iters, min_nodes=min_nodes,
                                        device=dev)
            costs.append(info["cost"])
        return x, _landmarks.build(centers, labels, x, starts=sessions, device=dev, **landmark_kw), costs

    def align_to_map(self, centers, labels, poses, lm, keep=None, radii=(2.0, 0.75), iters=10, min_nodes=6, min_matched=None,
                     tau_z=None):
        """Align scans to a landmark map from approximate poses (landmarks.align): one call per gate of
        the schedule `radii` (metres, wide to narrow), each starting from the poses of the one before; in a call every
        node takes the nearest landmark of its label inside the gate and the scan is re-fitted rigidly to its matches,
        `iters` times, every scan on its own.  The scans need not be part of the map, and the map is not changed.
        centers [Q,N,3], labels [Q,N]: the packed node arrays of the scans; poses: KITTI rows [Q,12] or planar [Q,4] in
        the frame of the map - what localize returned, odometry carried from a localised scan, a stored pose; lm: the
        dict of landmark_map; keep: a mask over its landmarks (landmarks.select; None: all); min_matched: a scan is
        accepted with that many matches at the end (None: min_nodes); tau_z: the height tolerance (None: the default of
        landmarks.build).
        -> (planar poses f64 [Q,4] device tensor, info dict of numpy arrays from the last call: matched, live, steps,
        flags, rms, node_landmark (-2 = a live node no landmark explains: an object the map does not know, -1 = dead), and
        accept = matched >= min_matched)."""
        from . import landmarks as _landmarks
        dev = self.engine().device
        x = poses if isinstance(poses, torch.Tensor) and poses.dim() == 2 and poses.shape[1] == 4 else _planar(poses)
        x = _engine._on(x, dev, torch.float64)
        radii = [float(r) for r in np.atleast_1d(np.asarray(radii, dtype=np.float64))]
        if not radii:
            raise ValueError("align_to_map: the gate schedule is empty")
        info = None
        for r in radii:
            x, info = _landmarks.align(centers, labels, x, lm, use=keep, radius=r, iters=iters, min_nodes=min_nodes,
                                       tau_z=_landmarks.DEFAULT_TAU_Z if tau_z is None else tau_z, device=dev)
        info["accept"] = info["matched"] >= (int(min_nodes) if min_matched is None else int(min_matched))
        return x, info

    def track_in_map(self, centers, labels, odom, init, lm, use=None, starts=None, radii=(2.0, 0.75), reacquire_radii=(8.0,),
                     iters=10, min_nodes=6, min_matched=10, max_shift=float("inf"), start_lost=False, tau_z=None):
        """Track drives through a landmark map (landmarks.track): the run-time use of the map.  One initial
        pose per drive - what localize returned - then the drive's own odometry, and the map correcting it scan by scan, in
        ONE call: scan i starts from the tracked pose of scan i - 1 moved by the odometry between the two, is aligned to
        the map through the gates `radii` (align_to_map's schedule, on that one scan) and accepted, or LOST - fewer than
        min_matched matches at the end, or fitted more than max_shift metres from where the odometry put it: then it keeps
        the predicted pose, so the track dead-reckons on, and the next scan runs the wider gates reacquire_radii first.
        centers [Q,N,3], labels [Q,N]: the packed node arrays of the drives' scans, in order; odom: KITTI rows [Q,12] or
        planar [Q,4] in a frame of the drive's own (only the motion between consecutive scans is read); starts: the first
        scan of every drive (None: one drive); init: the pose of every drive's first scan in the frame of the map, KITTI
        rows or planar [n_drives,4]; lm: the dict of landmark_map or update_map; use: a mask over its landmarks
        (landmarks.select; None: all); start_lost: run the wide gates on a drive's first scan too (an uncertain init).
        A TRACK THAT STAYS LOST - info["lost"] up to its last scan, num[2] growing from call to call - has left the reach
        of its gates: dead reckoning drifts on without bound, and only localize can place it again.  THE ROWS OF LOST
        SCANS MUST NOT BE FED TO update_map: their pose is a prediction and their node_landmark what a failed alignment
        saw; fold in the scans with ~info["lost"] only.
        -> (planar poses f64 [Q,4] device tensor, info dict of numpy arrays: pred [Q,4] (the prediction of every scan),
        matched, live, steps, flags (landmarks.TRACK_*), lost bool [Q], rms, node_landmark [Q,N], num = (scans tracked,
        scans lost, longest run of lost scans, drives))."""
        from . import landmarks as _landmarks
        dev = self.engine().device

        def planar(p):
            if not (isinstance(p, torch.Tensor) and p.dim() == 2 and p.shape[1] == 4):
                p = _planar(np.atleast_2d(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)))
            return _engine._on(p, dev, torch.float64)
        return _landmarks.track(centers, labels, planar(odom), planar(init), lm, use=use, starts=starts, radii=radii,
                                reacquire_radii=reacquire_radii, iters=iters, min_nodes=min_nodes, min_matched=min_matched,
                                max_shift=max_shift, start_lost=start_lost,
                                tau_z=_landmarks.DEFAULT_TAU_Z if tau_z is None else tau_z, device=dev)

    def relocalize_in_map(self, centers, labels, lm, use=None, radii=(2.0, 0.75), iters=10, min_nodes=6, min_inliers=12,
                          ratio=0.7, radius_in=0.75, tau_edge=0.5, min_base=5.0, max_base=30.0, max_hyp=65536, sep=10.0,
                          tau_z=None):
        """Relocalise scans in a landmark map with NO prior pose (landmarks.relocalize): the answer to
        "where am I?" from the landmarks alone - no scan of the map, no descriptor, no initial pose.  Every pair of nodes
        of a scan min_base..max_base metres apart is laid on the pairs of landmarks of their labels whose distance agrees
        within tau_edge; the pose under which the most nodes lie within radius_in of a landmark of their label wins, is
        FOUND with min_inliers of them, and is refined through the gates `radii` (align_to_map's schedule, on that scan).
        centers [Q,N,3], labels [Q,N]: the packed node arrays of the scans; lm: the dict of landmark_map or update_map;
        use: a mask over its landmarks (landmarks.select; None: all) - it also restricts the search to a part of the
        map; max_hyp: the hypotheses after which no further pair of nodes is started; sep: how many metres away another
        place is.
        A map that repeats itself - an avenue, a car park - answers with one of several places.  info["inliers_other"]
        is the best count more than `sep` from the answer; a scan is AMBIGUOUS when inliers_other >= ratio * inliers.
        A SCAN THAT IS AMBIGUOUS OR NOT FOUND MUST NOT SEED track_in_map (its `init`) AND MUST NOT BE FED TO
        update_map: its pose is NaN or one candidate among equals; wait for a scan that is found and unambiguous.
        -> (planar poses f64 [Q,4] device tensor, NaN where not found; info dict of numpy arrays: found, ambiguous bool
        [Q], inliers, inliers_other, coarse, other [Q,4], win [Q,4], hypotheses, matched, live, steps, flags
        (landmarks.RELOC_*), rms, node_landmark [Q,N], num = (scans found, scans truncated, scans without a hypothesis,
        0))."""
        from . import landmarks as _landmarks
        x, info = _landmarks.relocalize(centers, labels, lm, use=use, radius_in=radius_in, radii=radii,
                                        tau_z=_landmarks.DEFAULT_TAU_Z if tau_z is None else tau_z, tau_edge=tau_edge,
                                        min_base=min_base, max_base=max_base, max_hyp=max_hyp, min_inliers=min_inliers, sep=sep,
                                        iters=iters, min_nodes=min_nodes, device=self.engine().device)
        info["ambiguous"] = info["found"] & (info["inliers_other"] >= float(ratio) * info["inliers"])
        return x, info

    def update_map(self, centers, labels, poses, lm, session, node_base=None, radius=0.75, tau_z=None):
        """Fold the scans of a further drive into a landmark map (landmarks.update).  Every node is
        associated with the nearest landmark of its label within `radius` of the WHOLE map - one landmarks.align call
        with iters=0 and no keep mask, because a landmark seen once must be able to grow - and becomes one more
        observation of it; the live nodes without a landmark are fused among themselves (same radius, tau_z) into new
        landmarks behind the old ones.  Old landmarks keep their ids and never merge.
        ALIGN FIRST (align_to_map) and pass the poses it returned: from poses 0.3 m off, only 0.6 of the nodes of
        permanent objects fall within 0.75 m of their landmark, and the rest enter the map as duplicates beside it.
        centers [Q,N,3], labels [Q,N]; poses: KITTI rows [Q,12] or planar [Q,4] in the frame of the map; lm: the dict
        of landmark_map or of an earlier update_map; session: the number of the drive in the map (its bit in
        `sessions`; the scans are one session); node_base: the flat index the map gives the drive's first node (`first`
        of a new landmark; None: the largest `first` of the map + 1, rounded up to a multiple of N).
        -> the dict of landmarks.update: the records of the updated map, node_landmark [Q,N] of these scans,
        num_landmarks, live_nodes, observed, new_nodes."""
        from . import landmarks as _landmarks
        dev = self.engine().device
        x = poses if isinstance(poses, torch.Tensor) and poses.dim() == 2 and poses.shape[1] == 4 else _planar(poses)
        x = _engine._on(x, dev, torch.float64)
        tz = _landmarks.DEFAULT_TAU_Z if tau_z is None else tau_z
        assoc = _landmarks.align_async(centers, labels, x, lm, radius=radius, tau_z=tz, iters=0, device=dev)["node_landmark"]
        if node_base is None:
            first, n = torch.as_tensor(lm["first"]), int(assoc.shape[1])
            node_base = 0 if first.numel() == 0 or n == 0 else (int(first.max()) + n) // n * n
        return _landmarks.update(centers, labels, x, assoc, lm, session_base=int(session), node_base=int(node_base),
                                 radius=radius, tau_z=tz, device=dev)

    def map_persistence(self, centers, labels, poses, lm, node_landmark=None, max_range=50.0, margin=2.0, min_expected=5,
                        max_seen_ratio=0.3, radius=0.75, tau_z=None):
        """What a drive should have seen of a landmark map and what it saw (landmarks.persist): per
        landmark the scans that had it within their view range or observed it (expected) and the scans with a node on
        it (seen), and keep = False for the landmarks the drive expected at least min_expected times and saw in less
        than max_seen_ratio of them - the parked car that has left.  The map is not changed: pass keep to
        landmarks.select, align_to_map or landmarks.virtual_scans.  A scan's view range is the range of its farthest
        live node, at most max_range, less margin (metres).  There is no occlusion model.
        ALIGN FIRST (align_to_map) and pass the poses it returned, as for update_map: from poses 0.3 m off, nodes of
        permanent objects miss their landmarks and the landmarks count as unseen.  Run it on the drive JUST FOLDED IN,
        on the UPDATED map, with the node_landmark that update_map returned: the drive's new landmarks are then seen by
        it, and a lifetime ratio cannot tell "gone since last week" from "new since last week".
        centers [Q,N,3], labels [Q,N]; poses: KITTI rows [Q,12] or planar [Q,4] in the frame of the map; lm: the dict
        of landmark_map or update_map; node_landmark [Q,N]: the association of the nodes with lm (None: as update_map
        makes it - one landmarks.align call with iters=0 and no use mask, gate `radius`, tau_z).
        -> the dict of landmarks.persist: expected, seen, keep per landmark, scan_expected, scan_seen, scan_live, flags,
        view per scan, num."""
        from . import landmarks as _landmarks
        dev = self.engine().device
        x = poses if isinstance(poses, torch.Tensor) and poses.dim() == 2 and poses.shape[1] == 4 else _planar(poses)
        x = _engine._on(x, dev, torch.float64)
        if node_landmark is None:
            tz = _landmarks.DEFAULT_TAU_Z if tau_z is None else tau_z
            node_landmark = _landmarks.align_async(centers, labels, x, lm, radius=radius, tau_z=tz, iters=0,
                                                   device=dev)["node_landmark"]
        return _landmarks.persist(centers, labels, x, node_landmark, lm, radius=radius, max_range=max_range, margin=margin,
                                  min_expected=min_expected, max_seen_ratio=max_seen_ratio, device=dev)

    def compact_map(self, lm, keep=None, radius=0.75, tau_z=None):
        """Compact a landmark map on its records alone (landmarks.compact): the landmarks `keep` drops -
        map_persistence's keep, or any mask; None: none - are removed, duplicates of one label within `radius` of one
        another are fused as if their observations had been, and the rest are renumbered densely in their old order,
        bit for bit what they were.  No node array is read.  lm: the dict of landmark_map, update_map or merge_maps.
        -> the dict of landmarks.merge: the six records, num_landmarks, old_to_new (landmarks.remap carries a
        node_landmark array through it), dropped, fused."""
        from . import landmarks as _landmarks
        return _landmarks.compact(lm, keep=keep, radius=radius, tau_z=tau_z, device=self.engine().device)

    def register_maps(self, a, b, use_a=None, use_b=None, min_count=3, ratio=0.7, **relocalize_kw):
        """The planar pose that carries the frame of landmark map `b` into the frame of map `a`, from the landmarks alone
        (DESIGN.md §36): b's selected landmarks - count >= min_count, and use_b where given - become ONE query scan
        (their centres less their planar mean, formed in float64, then float32) that landmarks.relocalize places among
        a's selected landmarks with no prior pose; the answer is composed with the centring shift by the `a o b` rule
        of sgpr_landmark_track.h.  A host-level composition of existing calls with ONE synchronisation of its own - b's
        selected records cross to the host in one transfer - before landmarks.relocalize, which reads its answer back.
        A MAP b TOO LARGE TO BE ONE SCAN - relocalize pairs every two of its nodes min_base..max_base apart, and stops
        starting pairs at max_hyp hypotheses - IS THE CALLER'S TO CUT WITH use_b: a part of b that overlaps a is enough,
        the pose holds for all of b.  relocalize_kw: radii, min_inliers, radius_in, tau_edge, min_base, max_base,
        max_hyp, sep, iters, min_nodes, tau_z of landmarks.relocalize.
        -> (pose f64 [4] numpy (c, s, X, Y), or None when the scan is not found or another place holds at least `ratio`
        of its inliers; info: found, ambiguous, inliers, inliers_other, hypotheses, nodes (the landmarks of b used))."""
        from . import landmarks as _landmarks
        dev = self.engine().device
        pick_a = _landmarks.select(a, min_count=min_count, keep=use_a)
        pick_b = _landmarks.select(b, min_count=min_count, keep=use_b)
        # b's centres, labels and mask cross to the host together: one transfer, one synchronisation
        where = pick_b.device
        packed = torch.cat((torch.as_tensor(b["center"]).to(device=where, dtype=torch.float64).reshape(-1, 3),
                            torch.as_tensor(b["label"]).to(device=where, dtype=torch.float64).reshape(-1, 1),
                            pick_b.to(torch.float64).reshape(-1, 1)), dim=1).detach().cpu().numpy()
        idx = np.flatnonzero(packed[:, 4] != 0)
        cen, lab = packed[idx, :3], packed[idx, 3].astype(np.int32)
        mean = cen[:, :2].mean(axis=0) if cen.shape[0] else np.zeros(2)
        q = cen.copy()
        q[:, :2] -= mean
        x, info = _landmarks.relocalize(q.astype(np.float32)[None], lab[None], a, use=pick_a, device=dev, **relocalize_kw)
        found = bool(info["found"][0])
        ambiguous = found and bool(info["inliers_other"][0] >= float(ratio) * info["inliers"][0])
        out = {"found": found, "ambiguous": ambiguous, "inliers": int(info["inliers"][0]),
               "inliers_other": int(info["inliers_other"][0]), "hypotheses": int(info["hypotheses"][0]), "nodes": int(cen.shape[0])}
        if not found or ambiguous:
            return None, out
        tc, ts, tx, ty = (np.float64(v) for v in x[0].cpu().numpy())
        bx, by = np.float64(-mean[0]), np.float64(-mean[1])
        # a o b with b = (1, 0, bx, by): every product, sum and difference rounded once, in the order written
        one, zero = np.float64(1.0), np.float64(0.0)
        pose = np.array([tc * one - ts * zero, ts * one + tc * zero, (tc * bx - ts * by) + tx, (ts * bx + tc * by) + ty])
        return pose, out

    def merge_maps(self, a, b, pose=None, keep_a=None, keep_b=None, session_shift=None, first_base=None, radius=0.75, tau_z=None,
                   **register_kw):
        """Join two landmark maps that were built apart - two vehicles, two days - on their records alone
        (landmarks.merge): records of one label within `radius` fuse, inside a map and across the two,
        as if their observations had been fused; no node array is read.  pose: planar (c, s, X, Y) that carries b's
        frame into a's; None: the maps share a frame; "register": register_maps(a, b, **register_kw) finds it, and the
        call raises where that answers None.  keep_a, keep_b: masks that drop landmarks first (None: none);
        session_shift: b's session bits move up by this (None: the number of session bits a uses); first_base: added to
        b's `first` (None: the largest `first` of a + 1).
        -> the dict of landmarks.merge - the records of the joined map, num_landmarks, old_to_new [L_a + L_b] (b's
        landmark j is entry L_a + j), dropped, fused - plus pose (numpy [4], or None)."""
        from . import landmarks as _landmarks
        if isinstance(pose, str):
            if pose != "register":
                raise ValueError("merge_maps: pose is a planar pose, None or \"register\"")
            pose, info = self.register_maps(a, b, use_a=keep_a, use_b=keep_b, **register_kw)
            if pose is None:
                raise RuntimeError("merge_maps: map b could not be registered in map a (%s)" % (info,))
        elif register_kw:
            raise TypeError("merge_maps: %s only go with pose=\"register\"" % ", ".join(sorted(register_kw)))
        if session_shift is None:
            sess = torch.as_tensor(a["sessions"].view(np.int64) if isinstance(a["sessions"], np.ndarray) and
                                   a["sessions"].dtype == np.uint64 else a["sessions"]).to(torch.int64).reshape(-1)
            # the highest bit in use is that of the largest mask as an unsigned number: bit 63 where a mask is negative
            # as int64, else the bit length of the maximum - two reductions where the masks are, one read-back
            session_shift = 0
            if sess.numel():
                low, high = torch.stack((sess.min(), sess.max())).tolist()
                session_shift = 64 if low < 0 else int(high).bit_length()
        if first_base is None:
            first = torch.as_tensor(a["first"])
            first_base = 0 if first.numel() == 0 else max(int(first.max()) + 1, 0)
        out = _landmarks.merge(a, b, keep_a=keep_a, keep_b=keep_b, pose=pose, session_shift=int(session_shift),
                               first_base=int(first_base), radius=radius, tau_z=tau_z, device=self.engine().device)
        out["pose"] = None if pose is None else np.asarray(pose.detach().cpu() if isinstance(pose, torch.Tensor) else pose,
                                                            dtype=np.float64).reshape(4)
        return out

    def hard_pairs(self, pooled_rows, pooled_cols, col_pose, k=1, positives=False, d_pos=3.0, d_neg=20.0, window=-1,
                   row0=0, causal=False, row_self=None, row_pose=None):
        """The k hardest negatives (or, positives=True, positives) per row of pooled_rows x pooled_cols without forming
        the matrix (engine.Engine.score_mine) -> (values f32 [R,k], indices i32 [R,k]) on the device."""
        return self.engine().score_mine(pooled_rows, pooled_cols, col_pose, k=k, positives=positives, d_pos=d_pos,
                                        d_neg=d_neg, window=window, row0=row0, causal=causal, row_self=row_self,
                                        row_pose=row_pose)

    def loop_closures_above(self, pooled_rows, pooled_cols, threshold, window=-1, row0=0, causal=False, row_self=None,
                            capacity=None, seq_len=1, seq_reverse="both", seq_slopes=None, row_sessions=None,
                            col_sessions=None, min_terms=1):
        """Every pair of pooled_rows x pooled_cols scoring >= threshold, without forming the matrix
        (engine.Engine.score_above) -> (rows i32 [n], cols i32 [n], values f32 [n], row_ptr i64 [R+1]) on the device.
        seq_len > 1: rows and columns are consecutive scans and the sequence-matched score is thresholded
        (engine.Engine.score_seq_above; seq_reverse False / True / "both") -> (rows, cols, values, dirs u8 [n], row_ptr).
        seq_slopes (engine.seq_paths' slopes), row_sessions / col_sessions (the first row / column of every session of a
        stacked multi-session map) or min_terms > 1: the session-aware path-set score, folded over the candidates with
        at least min_terms terms (engine.Engine.score_session_above) -> (rows, cols, values, codes u8 [n], row_ptr)."""
        if seq_slopes is not None or row_sessions is not None or col_sessions is not None or int(min_terms) != 1:
            paths = None if seq_slopes is None else _engine.seq_paths(int(seq_len), seq_slopes)
            return self.engine().score_session_above(pooled_rows, pooled_cols, int(seq_len), threshold, paths,
                                                     row_sessions=row_sessions, col_sessions=col_sessions,
                                                     min_terms=int(min_terms), window=window, row0=row0, causal=causal,
                                                     row_self=row_self, reverse=seq_reverse, capacity=capacity)
        if int(seq_len) != 1:
            return self.engine().score_seq_above(pooled_rows, pooled_cols, int(seq_len), threshold, window=window,
                                                 row0=row0, causal=causal, row_self=row_self, reverse=seq_reverse,
                                                 capacity=capacity)
        return self.engine().score_above(pooled_rows, pooled_cols, threshold, window=window, row0=row0, causal=causal,
                                         row_self=row_self, capacity=capacity)

    def evaluate_pooled(self, pooled_rows, pooled_cols, pose_xz=None, p_thresh=3.0, n_thresh=20.0, gt=None, row0=0,
                        want_auc=True, seq_len=1, seq_reverse="both"):
        """(F1-max, ROC area, counting passes) of the pairs pooled_rows x pooled_cols without forming the matrix
        (metrics.pr_roc_pooled): ground truth from planar poses [.,2] or explicit int8 labels [R,M].
        seq_len > 1: of their sequence-matched score (metrics.pr_roc_seq_pooled)."""
        from . import metrics
        if int(seq_len) != 1:
            return metrics.pr_roc_seq_pooled(self.engine(), pooled_rows, pooled_cols, int(seq_len), pose_xz=pose_xz,
                                             p_thresh=p_thresh, n_thresh=n_thresh, gt=gt, row0=row0, reverse=seq_reverse,
                                             want_auc=want_auc)
        return metrics.pr_roc_pooled(self.engine(), pooled_rows, pooled_cols, pose_xz=pose_xz, p_thresh=p_thresh,
                                     n_thresh=n_thresh, gt=gt, row0=row0, want_auc=want_auc)

    def forward_packed(self, centers_1, labels_1, centers_2, labels_2, validate=True):
        """Faithful per-pair scoring of packed graphs: both sides embedded, then the tail.
        validate (default): synchronise and raise SgprError if the kernel saw a label outside [-1, L) (the reference
        raises KeyError, sg_net.py:277) or a broken node_cap promise; pass False on latency-critical paths whose
        inputs were checked when they were packed."""
        b = labels_1.shape[0]
        c = torch.cat((torch.as_tensor(centers_1), torch.as_tensor(centers_2)), dim=0)
        l = torch.cat((torch.as_tensor(labels_1), torch.as_tensor(labels_2)), dim=0)
        pooled, att, _ = self.embed(c, l, want_att=True)
        score = self.score_pooled(pooled[:b], pooled[b:])
        if validate:
            self.engine().check_status()
        return score, att[:b].unsqueeze(-1), att[b:].unsqueeze(-1)


def subsample_indices(centers, nodes, node_num):
    """The engine's documented, SEEDED rule for graphs with more than node_num nodes.

    The reference draws `np.random.choice(n, node_num, replace=False)` from the global, unseeded NumPy state and sorts
    the indices (sg_net.py:252-256), so two runs of the reference score such a graph differently.  Here the draw is
    `np.random.default_rng(seed).choice(n, node_num, replace=False)`, sorted, with
    `seed = crc32(float64 centres bytes + int64 label bytes)`: a function of the graph alone, hence the same subset in
    every pair, batch, process and rank."""
    c = np.ascontiguousarray(np.asarray(centers, dtype=np.float64).reshape(len(nodes), 3))
    l = np.ascontiguousarray(np.asarray(nodes).astype(np.int64).reshape(-1))
    seed = zlib.crc32(l.tobytes(), zlib.crc32(c.tobytes()))
    idx = np.random.default_rng(seed).choice(len(nodes), int(node_num), replace=False)
    idx.sort()
    return idx


def pack_graph(centers, nodes, node_num, number_of_labels=12, strict=False):
    """One side of transfer_to_torch (sg_net.py:250-272) in packed form.

    Returns (centers f32 [node_num,3], labels i32 [node_num]); padded slots have
    centre 0 / label -1.  A label outside [0, L) raises KeyError like
    `self.global_labels[node]` (sg_net.py:277).  A graph with more than node_num
    nodes is subsampled like the reference does (sg_net.py:252-256) but with the
    seeded rule of `subsample_indices` (a warning names the graph size);
    strict=True rejects it instead.  Note that such a graph has no padded slot, so
    its one-hot kNN ties are broken by the implementation: the
    reference's own CPU and CUDA results already differ there."""
    n = len(nodes)
    if n > node_num:
        if strict:
            raise ValueError("graph has %d nodes > node_num=%d (strict packing)" % (n, node_num))
        warnings.warn("graph with %d nodes subsampled to node_num=%d (seeded rule, sg_pr_amd.sg_net.subsample_indices)"
                      % (n, node_num), stacklevel=2)
        keep = subsample_indices(centers, nodes, node_num)
        centers = np.asarray(centers, dtype=np.float64).reshape(n, 3)[keep]
        nodes = np.asarray(nodes).reshape(-1)[keep]
        n = int(node_num)
    lab = np.asarray(nodes).astype(np.int64).reshape(-1)
    bad = (lab < 0) | (lab >= number_of_labels)
    if bad.any():
        raise KeyError(int(lab[bad][0]))
    c = np.zeros((node_num, 3), dtype=np.float32)
    l = -np.ones(node_num, dtype=np.int32)
    if n:
        c[:n] = np.asarray(centers, dtype=np.float64).reshape(n, 3)
        l[:n] = lab
    return c, l


class SGTrainer(object):
    """Inference half of the reference harness (sg_net.py:141-206, 241-310, 434-525)."""

    GRAPH_CACHE_MAX = 65536      # packed graphs kept by _load_graph (LRU): ~110 MB at node_num 100, > 14 KITTI-00s

    def __init__(self, args, train=True):
        if train:
            raise NotImplementedError("training (SGTrainer.fit) is out of scope of the MI355X engine; "
                                      "construct with train=False")
        self.args = args
        self.model_pth = self.args.model
        self.initial_label_enumeration(train)
        self.setup_model(train)
        self._graph_cache = OrderedDict()            # path -> packed graph, least recently used first

    def initial_label_enumeration(self, train=True):
        """sg_net.py:178-206 - twelve SemanticKITTI-derived node classes."""
        self.global_labels = {val: index for index, val in enumerate(range(12))}
        self.number_of_labels = len(self.global_labels)
        self.keepnode = getattr(self.args, "keep_node", 1)

    def setup_model(self, train=True):
        """sg_net.py:158-176 - build SG, load the DataParallel checkpoint (strip `module.`)."""
        self.model = SG(self.args, self.number_of_labels)
        if (not train) and self.model_pth != "":
            print("loading model: ", self.model_pth)
            state_dict = torch.load(self.model_pth, map_location="cpu")
            new_state_dict = OrderedDict()
            for k, v in state_dict.items():
                new_state_dict[k[7:] if k.startswith("module.") else k] = v
            self.model.load_state_dict(new_state_dict)
        self.model.eval()

    # ------------------------------------------------------------------ host packing
    def _load_graph(self, path):
        """Parse one graph JSON once and keep its packed form (the reference re-reads and
        re-pads every graph for every pair it appears in: utils.py:27-28, sg_net.py:250-299)."""
        g = self._graph_cache.get(path)
        if g is None:
            d = read_graph(path)
            c, l = pack_graph(d["centers"], d["nodes"], int(self.args.node_num), self.number_of_labels)
            g = (c, l, d["pose"])
            self._graph_cache[path] = g
            while len(self._graph_cache) > self.GRAPH_CACHE_MAX:       # bounded: 1.7 KB per packed graph at node_num 100
                self._graph_cache.popitem(last=False)
        else:
            self._graph_cache.move_to_end(path)
        return g

    def target_from_distance(self, distance):
        """sg_net.py:302-309."""
        if distance <= self.args.p_thresh:
            return 1.0
        if distance >= 20:
            return 0.0
        print("distance error: ", distance)
        exit(-1)

    def transfer_to_torch(self, data, training=True):
        """sg_net.py:241-310 - pair dictionary -> dense `features_1/2` [(3+L), node_num] + target.
        Unlike the reference this does not mutate `data`."""
        if training:
            raise NotImplementedError("augmentation / training branch is out of scope")
        new_data = dict()
        for side in ("1", "2"):
            cen, nod = data["centers_" + side], data["nodes_" + side]
            if len(nod) > int(self.args.node_num):                      # sg_net.py:252-256, seeded (subsample_indices)
                keep = subsample_indices(cen, nod, int(self.args.node_num))
                cen = np.asarray(cen, dtype=np.float64).reshape(len(nod), 3)[keep]
                nod = np.asarray(nod).reshape(-1)[keep]
            c, l = pack_graph(cen, nod, int(self.args.node_num), self.number_of_labels)
            onehot = np.zeros((l.shape[0], self.number_of_labels), dtype=np.float64)
            real = l >= 0
            onehot[np.nonzero(real)[0], l[real]] = 1.0
            centers64 = np.zeros((l.shape[0], 3), dtype=np.float64)
            n = len(nod)
            centers64[:n] = np.asarray(cen, dtype=np.float64).reshape(n, 3)
            new_data["features_" + side] = np.concatenate((centers64, onehot), axis=1).T
        new_data["target"] = self.target_from_distance(data["distance"])
        return new_data

    # ------------------------------------------------------------------ evaluation entry points
    def eval_pair(self, pair_file):
        """sg_net.py:434-457 - one pair dictionary -> (prediction, att_weights_1, att_weights_2)."""
        data = self.transfer_to_torch(pair_file, False)
        data_torch = {
            "features_1": torch.FloatTensor(np.array([data["features_1"]])),
            "features_2": torch.FloatTensor(np.array([data["features_2"]])),
        }
        self.model.eval()
        r1, r2, r3 = self.model(data_torch)
        return (r1.cpu().detach().numpy().reshape(-1), r2.cpu().detach().numpy().reshape(-1),
                r3.cpu().detach().numpy().reshape(-1))

    def eval_batch_pair(self, batch):
        """sg_net.py:503-525 - list of [path_1, path_2] -> (pred float32 [B], gt float64 [B])."""
        self.model.eval()
        n = int(self.args.node_num)
        b = len(batch)
        centers = np.empty((2 * b, n, 3), dtype=np.float32)
        labels = np.empty((2 * b, n), dtype=np.int32)
        batch_target = []
        for i, graph_pair in enumerate(batch):
            c1, l1, pose1 = self._load_graph(graph_pair[0])
            c2, l2, pose2 = self._load_graph(graph_pair[1])
            centers[i], labels[i] = c1, l1
            centers[b + i], labels[b + i] = c2, l2
            batch_target.append(self.target_from_distance(pose_distance(pose1, pose2)))
        prediction, _, _ = self.model.forward_packed(centers[:b], labels[:b], centers[b:], labels[b:])
        prediction = prediction.cpu().detach().numpy().reshape(-1)
        gt = np.array(batch_target).reshape(-1)
        return prediction, gt

    def eval_batch_pair_data(self, batch):
        """sg_net.py:480-501 - like eval_batch_pair but on in-memory pair dictionaries."""
        self.model.eval()
        f1, f2, tgt = [], [], []
        for graph_pair in batch:
            data = self.transfer_to_torch(graph_pair, False)
            f1.append(data["features_1"])
            f2.append(data["features_2"])
            tgt.append(data["target"])
        data = {"features_1": torch.FloatTensor(np.array(f1)), "features_2": torch.FloatTensor(np.array(f2))}
        prediction, _, _ = self.model(data)
        return prediction.cpu().detach().numpy().reshape(-1), np.array(tgt).reshape(-1)

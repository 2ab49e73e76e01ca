"""A place database for loop-closure retrieval: the pooled vectors of every graph added so far, on the device, queried
with sgpr_score_topk - the k best matches per query, no similarity matrix at any size.

    db = PlaceDatabase(model)
    ids = db.add(centers, labels)                      # embed (ordered launch), append; -> new ids
    vals, idx = db.query(centers, labels, k=1, window=50, causal=True)   # new graphs: frames len(db), len(db) + 1, ...
    vals, idx = db.query_ids(ids, k=4, window=50)      # members: row_self = their ids
    rows, cols, vals, row_ptr = db.query_ids_above(ids, 0.9, window=50)   # every member scoring >= 0.9
    vals, idx, dirs = db.query_seq(centers, labels, seq_len=8, k=4, window=50, causal=True)   # sequence-matched
    vals, idx, dirs = db.query_ids_seq(first, count, seq_len=8, k=4, window=50)               # a run of members
    rows, cols, vals, dirs, row_ptr = db.query_seq_above(centers, labels, seq_len=8, threshold=0.9, window=50, causal=True)
    db.save("map.npz"); db = PlaceDatabase.load("map.npz", model)

A vector costs 128 bytes of device memory (the matrix of a 100 k-graph map would be 40 GB).  The file keeps the vectors,
the architecture and a sha256 of the checkpoint's weight blob: vectors of one checkpoint are meaningless to another, so
`load` refuses them.

    python -m sg_pr_amd.place_db config.yml [--k K] [--window W] [--causal] [--threshold T] [--hard K]
                                            [--recall-percent P] [--seq-len L] [--seq-reverse {off,on,both}]
                                            [--verify] [--min-inliers I] [--consistent] [--distinct RHO] [--seq-slopes S,S,...]
                                            [--sessions N] [--optimize] [--save-poses FILE] [--landmarks] [--track] [--relocalize]
                                            [--update [--retire] [--compact]] [--merge-maps]

runs every `eva_batch.sequences` entry (packed and cached like graph_store): `<output_path>/<seq>_topk.npz` with
frame, indices [M,K], scores [M,K] and recall@1..K (K up to 4096); with --recall-percent P the lists hold
max(K, N) candidates, N = max(1, round(M * P / 100)), and the file adds recall_percent and recall_percent_n; with --threshold also `<seq>_above.npz` with every pair scoring
>= T (rows, cols, scores) and its precision / recall (metrics.precision_recall_at); with --hard K also `<seq>_hard.npz`
with every frame's K hardest negatives (highest scores at >= 20 m) and K hardest positives (lowest scores within
p_thresh), indices and scores (Engine.score_mine; the window applies to both), and the number of frames that have a
negative scoring above their best positive.  With --seq-len L (2..32) the lists of `<seq>_topk.npz` rank the
sequence-matched score (the mean along the diagonal of the last L frames of both trajectories, engine.Engine.seq_filter;
--seq-reverse: forward diagonals only (off), reverse only (on) or the larger of both, the default) and the file adds
seq_len and dirs [M,K] (0 forward, 1 reverse).  With --threshold and --seq-len L > 1 also `<seq>_seq_above.npz`: every
pair whose sequence-matched score is >= T (rows, cols, scores, dirs, precision, recall, seq_len; Engine.score_seq_above);
`<seq>_above.npz` stays the single-scan result.  With --verify the retrieved lists are verified geometrically on the
packed graphs (SG.verify_closures: planar consensus of the labelled centres, engine.verify_pairs): `<seq>_verify.npz` holds
per list slot inliers, inliers_refined, flags, refined [M,K,4] (c, s, tx, ty: row scan -> column scan), yaw, rmse, the
re-ranked lists indices_ranked (refined inliers descending, then score, then column) and accept (inliers_refined >=
--min-inliers, default 12); printed are recall@1 before and after re-ranking, the precision of the accepted closures
and the median yaw / translation error of the accepted true closures against the poses.  With --distinct RHO
(0..1024) the K best distinct places are retrieved as well - the peaks of the ranked score within RHO frames
(engine.Engine.score_peak_topk; --seq-len still chooses the score; choose RHO <= --window):
`<seq>_distinct.npz` holds frame, indices [M,K], scores [M,K], recall, radius (and seq_len, dirs); printed are
recall@1 and recall@K of the distinct lists beside the plain ones and the mean number of places per list (groups of
listed frames at most RHO apart) of both; with --verify the distinct lists are verified too (`<seq>_distinct_verify.npz`)
and the number of pairs verified in each mode is printed.  With --seq-len L > 1 and --seq-slopes 1,1/2,2/3,3/2,2 the
speed-tolerant lists are retrieved as well - the best mean over the paths of these slopes (engine.seq_paths,
engine.Engine.score_path_topk; --distinct composes): `<seq>_slopes.npz` holds frame, indices [M,K],
scores [M,K], codes [M,K] (direction bit | path << 1), paths [P,L], recall, seq_len (and radius); printed are
recall@1 and recall@K beside the unit-slope lists and the share of listed entries per path.  With --sessions N
(2..64) the sequence is also taken as a multi-session map: N consecutive near-equal sessions, session j starting at frame
(j * M) // N, stored with new_session() between them and queried through the session call (sums and the window stop at
session boundaries, engine.Engine.score_session_topk; --seq-len and --seq-slopes choose the score):
`<seq>_sessions.npz` holds frame, indices [M,K], scores [M,K], codes [M,K], session_starts, recall, recall_head,
recall_one_trajectory, recall_head_one_trajectory (and seq_len); printed are recall@1 and recall@K beside the
one-trajectory lists, and the same pair for the head rows alone - the frames fewer than --window scans after the start
of a session that has a predecessor.  All four are counted under the session rule for an allowed match
(metrics.recall_at_n with col_starts), so the two lists are judged on the same queries.  With --verify --consistent
[--max-trans M] [--max-yaw-deg D] [--lever-gain G] [--min-clique N] the accepted closures are also checked against one
another through the poses (SG.consistent_closures; with --sessions N within each pair of sessions):
`<seq>_consistent.npz` holds rows, cols, refined, consistent, rank, degree, group_size, session_starts and the counts;
printed are the number and the precision of the accepted closures before and after the selection.  With --optimize
[--save-poses FILE] on top of that the planar pose graph of the map - the sequence's poses as odometry, the consistent
closures as loop edges, the first scan fixed - is relaxed on the device (SG.optimize_map, posegraph.optimize, DESIGN.md
§25): printed are the closures and scans that took part, the trajectory error of the map against the poses before and
after (metrics.trajectory_error) and the iterations of the two stages; FILE gets the optimised poses [M,4] (.npy).
With --verify --localize [--loc-len L] [--min-support S] [--loc-max-trans M] [--loc-max-yaw-deg D] every scan is
localised in the sequence's own planar ground-truth poses from the candidates its list retrieved (SG.localize,
localize.localize; the window already keeps a scan's neighbours out of its list): the verified candidates
of the scan and of the L - 1 scans before it, carried forward by the poses as odometry, vote on its pose, and it counts as
localised with a support of at least S.  `<seq>_localize.npz` holds pose [M,4], support, live, winner, flags, spread,
accept, trans_m, yaw_deg, the records that went in (indices, refined, verify_flags, verify_accept) and the parameters;
printed are the share localised and the median and 95th-percentile translation and yaw error, and beside them the same
numbers for the best verified candidate taken alone.
With --landmarks [--lm-radius R] [--lm-tau-z Z] [--lm-min-sessions S] the nodes of every scan are fused into a landmark
map (SG.landmark_map, landmarks.build) on the poses the run ends with - the optimised ones after
--optimize, the sequence's own otherwise - with the sessions of --consistent --sessions N.  `<seq>_landmarks.npz` holds
center, label, count, first, sessions, spread per landmark, node_landmark [M,N], keep (seen by at least S sessions), the
poses and the parameters; printed are the landmarks with two or more observations, their sharpness, the share seen by
two or more sessions and the share of single observations (metrics.map_sharpness), and after --optimize the same four
on the poses before optimisation.
With --landmarks --refine [--refine-rounds R] [--refine-iters T] the poses the run ends with are first refined on the map's
own landmarks (SG.refine_map, landmarks.refine): R rounds (default 2) of landmark map, the landmarks with
two or more observations, T alternations (default 10) of centre means and closed-form pose fits, the first scan fixed.
Printed are landmarks, sharpness and shared before and after and the trajectory error against the sequence's own poses
before and after; the landmark map above is then the one on the refined poses, and --save-poses FILE gets them.

With --landmarks --align [--align-radii 2,0.75] [--align-iters T] every scan is then aligned to that landmark map
(SG.align_to_map, landmarks.align): one call of T iterations per gate of the schedule, every node to the
nearest landmark of its label inside the gate, the scan re-fitted to its matches.  With --localize the scans that were
given a pose start from it, every other scan - and without --localize every scan - from the pose the map was built on.
THE MAP HERE CONTAINS THE SCAN BEING ALIGNED: the figures say how well a scan sits on a map it helped to make, not how a
new drive would fare.  Printed are median and 95 % translation and yaw error against the sequence's own poses before and
after, the median share of a scan's live nodes that matched and the live nodes no landmark explains;
`<seq>_align.npz` holds poses, start [M,4], matched, live, steps, flags, rms, accept, node_landmark, radii, iters.

With --landmarks --sessions N --update the last of the N sessions is taken as a NEW DRIVE: a landmark map is built on
the other sessions (the sequence's own poses), the scans of the last are aligned to it with --align-radii and
--align-iters (all landmarks take part) and folded into it (SG.update_map, landmarks.update): matched
nodes become further observations of their landmarks, the others new landmarks behind the old ones.  Printed are the
landmarks before and after, the new landmarks, the observed and the new nodes, and the share of the updated landmarks
whose count is that of the landmark holding their first node in the map built on every session at once on the same poses;
`<seq>_update.npz` holds the records of the updated map, node_landmark of the new scans, num = (landmarks, live,
observed, new nodes), landmarks_before, batch_landmarks, same_count, poses, start, first_scan, session, node_base,
radii, iters.
With --retire [--view-range R] [--view-margin M] [--min-expected E] [--max-seen-ratio r] on top of that the drive just
folded in is tallied on the UPDATED map (SG.map_persistence, landmarks.persist) with the node_landmark the
update returned: a scan sees what lies within the range of its farthest node, at most R (default 50 m), less M (2 m); a
landmark the drive should have seen at least E times (5) and saw in less than r (0.3) of them is retired - a mask, the
records stay.  THERE IS NO OCCLUSION MODEL: a landmark hidden behind a lorry counts as missed, and M and r absorb that.
Printed are the landmarks in use (three or more observations) before and after retiring and the median over the scans of
landmarks seen / landmarks expected; `<seq>_persist.npz` holds expected, seen, keep per landmark, scan_expected,
scan_seen, scan_live, flags, view per scan, num = (retired, judged, eligible, scans with a view), in_use_before,
in_use_after, scan_ratio_median and the parameters.  Without --retire every output is as before.
With --compact after --update [--retire] the updated map is compacted on its records alone (SG.compact_map,
landmarks.merge): what --retire retired is removed (without --retire no mask is applied), records of one
label within --lm-radius of one another are fused, the rest are renumbered densely in their order.  Printed are the
landmarks before -> after, dropped and fused; `<seq>_compact.npz` holds the records, old_to_new, node_landmark of the new
scans carried through it, num = (landmarks, dropped by the mask, dropped as ineligible, fused) and landmarks_before.
With --landmarks --sessions N --merge-maps one landmark map is built per session on the sequence's own poses and the N
maps are merged left to right on their records (SG.merge_maps); printed beside the result is the landmark count of the
batch map of every session; `<seq>_merge.npz` holds the records, num, landmarks_per_session, fused, batch_landmarks and
same_count.  Without the two flags every output is as before.

With --landmarks --sessions N --track [--track-radii 2,0.75] [--reacquire-radii 8] [--min-matched M] the last of the N
sessions is TRACKED through the landmark map of the others (SG.track_in_map, landmarks.track): its first
scan starts from its localised pose (--localize, when that scan was localised) or its stored pose, every further scan
from the tracked pose of the one before moved by the sequence's own relative motion; a scan is aligned through the
gates of --track-radii (--align-iters rounds each), is lost with fewer than M matches (default 10) and then keeps its
prediction, and the scan after a lost one runs the gates of --reacquire-radii first.  Printed are the scans tracked and
lost, the longest run of lost scans and the median matched share; `<seq>_track.npz` holds poses, pred [Q,4], matched, live,
steps, flags, lost, rms, node_landmark, num = (tracked, lost, longest lost run, tracks), init, from_localize, first_scan,
session, radii, reacquire_radii, iters, min_matched, matched_share and the translation error against the sequence's own
poses.  Without --track every output is as before.

With --landmarks --sessions N --relocalize [--reloc-min-inliers I] [--reloc-max-base B] [--reloc-sep S] every scan of the
last of the N sessions is RELOCALISED in the landmark map of the others with no pose at all (SG.relocalize_in_map,
landmarks.relocalize): pairs of its nodes up to B metres apart (default 30) are laid on pairs of landmarks
of their labels, the pose with the most nodes on landmarks wins, is found with I of them (default 12) and is refined
through the gates of --align-radii (--align-iters rounds each); a scan is ambiguous when a pose more than S metres away
(default 10) collects 0.7 of the winner's count.  Printed are the share found, the share ambiguous and the median and
largest translation error of the found scans against the sequence's own poses; `<seq>_relocalize.npz` holds poses [Q,4],
found, ambiguous, inliers, inliers_other, coarse, other, win, hypotheses, matched, live, steps, flags, rms, node_landmark,
num = (found, truncated, without a hypothesis, 0), trans_m, first_scan, session and the parameters.  With --track and
without --localize the track starts from the relocalised pose of the session's first scan when that scan is found and
not ambiguous.  Without --relocalize every output is as before.
"""
import argparse
import math
import hashlib
import os

import numpy as np
import torch

from . import engine as _engine
from . import metrics

_DIMS = [f for f, _ in _engine.SgprDims._fields_]


def weights_sha256(model):
    """sha256 of the flat fp32 weight blob the engine is built from (include/sgpr.h order)."""
    return hashlib.sha256(_engine.blob_from_state_dict(model.state_dict()).tobytes()).hexdigest()


class PlaceDatabase:
    def __init__(self, model, capacity=1024):
        self.model = model
        self.eng = model.engine()
        self.k = int(model.args.K)
        self._buf = torch.empty(max(int(capacity), 1), self.eng.pw, dtype=torch.float32, device=self.eng.device)
        self.n = 0
        self._starts = [0]                                   # the first member of every session (new_session)

    @property
    def session_starts(self):
        """The first member id of every session, int32 [sessions] (one session: [0])."""
        return np.asarray(self._starts, dtype=np.int32)

    @property
    def _multi(self):
        return len(self._starts) > 1

    def new_session(self):
        """The members added from now on belong to a new session: a map recorded on an earlier drive ends here.  From
        the second session on every query goes through the session call (engine.Engine.score_session_topk, DESIGN.md
        §22): sums stop at session boundaries and the window excludes members of the query's own session only.
        A session without members is not opened twice.  -> the index of the current session."""
        if self.n > self._starts[-1]:
            if len(self._starts) >= _engine.SESSION_MAX:
                raise ValueError("new_session: more than %d sessions" % _engine.SESSION_MAX)
            self._starts.append(self.n)
        return len(self._starts) - 1

    def _no_sessions(self, what):
        if self._multi:
            hint = " (query_closures / query_ids_closures threshold a multi-session map)" if what.endswith("_above") else ""
            raise NotImplementedError("%s is not available on a database with more than one session%s" % (what, hint))

    def _session_rows(self, base, count):
        """the row table of members base .. base + count - 1 (a session that starts before `base` starts at row 0)"""
        return np.clip(self.session_starts.astype(np.int64) - base, 0, count).astype(np.int32)

    def __len__(self):
        return self.n

    @property
    def pooled(self):
        """[len, pooled width] device view of the stored vectors."""
        return self._buf[:self.n]

    def _embed(self, centers, labels):
        order, cap = self.eng.size_order(centers, labels, self.k)
        pooled = self.eng.embed(centers, labels, self.k, node_cap=cap, order=order)[0]
        self.eng.check_status()
        return pooled

    def append_pooled(self, pooled):
        """Store already embedded vectors [g, pooled width] -> their ids (int64 [g])."""
        pooled = self.eng._pooled(pooled, "pooled")
        g = pooled.shape[0]
        if self.n + g > self._buf.shape[0]:                  # geometric growth: amortised O(1) copies per vector
            cap = max(2 * self._buf.shape[0], self.n + g)
            buf = torch.empty(cap, self._buf.shape[1], dtype=torch.float32, device=self._buf.device)
            buf[:self.n] = self._buf[:self.n]
            self._buf = buf
        self._buf[self.n:self.n + g] = pooled
        ids = torch.arange(self.n, self.n + g, dtype=torch.int64)
        self.n += g
        return ids

    def add(self, centers, labels):
        """Embed packed graphs (centers [g,N,3], labels [g,N]) and append them -> their ids (int64 [g])."""
        return self.append_pooled(self._embed(centers, labels))

    def query(self, centers, labels, k=1, window=-1, causal=False, distinct=None):
        """The k best members for graphs that are NOT in the database, taken as frames len(db), len(db) + 1, ...
        -> (scores f32 [g,k], ids i32 [g,k]) on the device.  distinct=rho: the k best distinct places - score peaks
        within rho members (engine.Engine.score_peak_topk; the members are one trajectory, choose rho <= window).
        A causal query fed one scan at a time returns the lists of one offline causal call."""
        if self._multi:
            if distinct is not None:
                self._no_sessions("distinct=")
            return self.eng.score_session_topk(self._embed(centers, labels), self.pooled, 1, k=k, window=window,
                                               row0=self.n, causal=causal, col_sessions=self.session_starts,
                                               reverse=False)[:2]
        if distinct is not None:
            return self.eng.score_peak_topk(self._embed(centers, labels), self.pooled, int(distinct), k=k, window=window,
                                            row0=self.n, causal=causal)[:2]
        return self.eng.score_topk(self._embed(centers, labels), self.pooled, k=k, window=window, row0=self.n,
                                   causal=causal)

    def query_ids(self, ids, k=1, window=-1, causal=False, distinct=None):
        """The k best members for members `ids` (their own id is their frame: row_self = ids).  distinct=rho: the k
        best distinct places (query)."""
        ids = torch.as_tensor(ids, dtype=torch.int64).to(self._buf.device)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.n):
            raise IndexError("query_ids: ids must lie in [0, %d)" % self.n)
        rows = self.pooled.index_select(0, ids)
        if self._multi:
            if distinct is not None:
                self._no_sessions("distinct=")
            return self.eng.score_session_topk(rows, self.pooled, 1, k=k, window=window, causal=causal,
                                               row_self=ids.to(torch.int32), col_sessions=self.session_starts,
                                               reverse=False)[:2]
        if distinct is not None:
            return self.eng.score_peak_topk(rows, self.pooled, int(distinct), k=k, window=window, causal=causal,
                                            row_self=ids.to(torch.int32))[:2]
        return self.eng.score_topk(rows, self.pooled, k=k, window=window, causal=causal,
                                   row_self=ids.to(torch.int32))

    def _paths(self, seq_len, slopes):
        return _engine.seq_paths(int(seq_len), slopes)

    def query_seq(self, centers, labels, seq_len, k=1, window=-1, causal=False, reverse="both", pooled=None,
                  distinct=None, slopes=None):
        """Sequence-matched query for graphs that are NOT in the database, taken as the next frames len(db),
        len(db) + 1, ... of the trajectory the members form (or, pooled=, their already embedded vectors): the k best
        members by the score averaged along the last seq_len frames (engine.Engine.score_seq_topk), the database's last
        seq_len - 1 members serving as context rows -> (scores f32 [g,k], ids i32 [g,k], dirs u8 [g,k]).
        distinct=rho: the k best peaks of that score within rho members (engine.Engine.score_peak_topk).
        slopes (e.g. ("1", "1/2", "2")): the best mean over the paths of these slopes (engine.seq_paths,
        engine.Engine.score_path_topk) -> (scores, ids, codes u8: direction bit | path << 1).  Fed one scan at a time
        (causal) it returns the lists of one offline call iff window >= the paths' largest offset."""
        new = self._embed(centers, labels) if pooled is None else self.eng._pooled(pooled, "pooled")
        if self._multi:                                      # context rows: members of the current session only
            if distinct is not None:
                self._no_sessions("distinct=")
            ctx = min(int(seq_len) - 1, self.n - self._starts[-1])
            rows = torch.cat((self._buf[self.n - ctx:self.n], new)) if ctx > 0 else new
            return self.eng.score_session_topk(rows, self.pooled, int(seq_len),
                                               None if slopes is None else self._paths(seq_len, slopes),
                                               col_sessions=self.session_starts, k=k, window=window, row0=self.n - ctx,
                                               causal=causal, context=ctx, reverse=reverse)
        ctx = min(int(seq_len) - 1, self.n)
        rows = torch.cat((self._buf[self.n - ctx:self.n], new)) if ctx > 0 else new
        if slopes is not None:
            return self.eng.score_path_topk(rows, self.pooled, int(seq_len), self._paths(seq_len, slopes), k=k,
                                            radius=0 if distinct is None else int(distinct), window=window,
                                            row0=self.n - ctx, causal=causal, context=ctx, reverse=reverse)
        if distinct is not None:
            return self.eng.score_peak_topk(rows, self.pooled, int(distinct), seq_len=int(seq_len), k=k, window=window,
                                            row0=self.n - ctx, causal=causal, context=ctx, reverse=reverse)
        return self.eng.score_seq_topk(rows, self.pooled, int(seq_len), k=k, window=window, row0=self.n - ctx,
                                       causal=causal, context=ctx, reverse=reverse)

    def query_ids_seq(self, first, count, seq_len, k=1, window=-1, causal=False, reverse="both", distinct=None,
                      slopes=None):
        """Sequence-matched lists for the run of members first .. first + count - 1 (their ids are their frames), the
        up to seq_len - 1 members before `first` serving as context rows -> (scores, ids, dirs) [count, k].
        distinct=rho: the k best peaks of that score within rho members.  slopes: query_seq's -> (scores, ids, codes)."""
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.n:
            raise IndexError("query_ids_seq: first .. first + count must lie in [0, %d]" % self.n)
        ctx = min(int(seq_len) - 1, first)
        if self._multi:
            if distinct is not None:
                self._no_sessions("distinct=")
            return self.eng.score_session_topk(self._buf[first - ctx:first + count], self.pooled, int(seq_len),
                                               None if slopes is None else self._paths(seq_len, slopes),
                                               row_sessions=self._session_rows(first - ctx, ctx + count),
                                               col_sessions=self.session_starts, k=k, window=window, row0=first - ctx,
                                               causal=causal, context=ctx, reverse=reverse)
        if slopes is not None:
            return self.eng.score_path_topk(self._buf[first - ctx:first + count], self.pooled, int(seq_len),
                                            self._paths(seq_len, slopes), k=k,
                                            radius=0 if distinct is None else int(distinct), window=window,
                                            row0=first - ctx, causal=causal, context=ctx, reverse=reverse)
        if distinct is not None:
            return self.eng.score_peak_topk(self._buf[first - ctx:first + count], self.pooled, int(distinct),
                                            seq_len=int(seq_len), k=k, window=window, row0=first - ctx, causal=causal,
                                            context=ctx, reverse=reverse)
        return self.eng.score_seq_topk(self._buf[first - ctx:first + count], self.pooled, int(seq_len), k=k,
                                       window=window, row0=first - ctx, causal=causal, context=ctx, reverse=reverse)

    def query_ids_hard(self, ids, poses, k=1, positives=False, d_pos=3.0, d_neg=20.0, window=-1, causal=False):
        """The k hardest negatives (positives=True: positives) of stored members ids among all members
        (Engine.score_mine with row_self = ids); poses [len, 12] or [len, 2] of every member."""
        self._no_sessions("query_ids_hard")
        ids = torch.as_tensor(ids, dtype=torch.int64, device=self.eng.device)
        rows = self.pooled.index_select(0, ids)
        return self.eng.score_mine(rows, self.pooled, poses, k=k, positives=positives, d_pos=d_pos, d_neg=d_neg,
                                   window=window, causal=causal, row_self=ids.to(torch.int32))

    def query_above(self, centers, labels, threshold, window=-1, causal=False):
        """Every member scoring >= threshold for graphs that are NOT in the database (frames len(db), len(db) + 1, ...)
        -> (rows i32 [n], ids i32 [n], scores f32 [n], row_ptr i64 [g+1]) on the device (engine.Engine.score_above)."""
        self._no_sessions("query_above")
        return self.eng.score_above(self._embed(centers, labels), self.pooled, threshold, window=window, row0=self.n,
                                    causal=causal)

    def query_ids_above(self, ids, threshold, window=-1, causal=False):
        """Every member scoring >= threshold for members `ids` (row_self = ids)."""
        self._no_sessions("query_ids_above")
        ids = torch.as_tensor(ids, dtype=torch.int64).to(self._buf.device)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.n):
            raise IndexError("query_ids_above: ids must lie in [0, %d)" % self.n)
        rows = self.pooled.index_select(0, ids)
        return self.eng.score_above(rows, self.pooled, threshold, window=window, causal=causal,
                                    row_self=ids.to(torch.int32))

    def query_seq_above(self, centers, labels, seq_len, threshold, window=-1, causal=False, reverse="both", pooled=None):
        """query_seq's rows (new scans as the next frames, the last seq_len - 1 members as context rows) thresholded
        instead of ranked: every member whose sequence-matched score is >= threshold (engine.Engine.score_seq_above)
        -> (rows i32 [n], ids i32 [n], scores f32 [n], dirs u8 [n], row_ptr i64 [g+1]).  Fed one scan at a time it
        returns the pairs of one offline call, under query_seq's condition (causal, window >= seq_len - 1)."""
        self._no_sessions("query_seq_above")
        new = self._embed(centers, labels) if pooled is None else self.eng._pooled(pooled, "pooled")
        ctx = min(int(seq_len) - 1, self.n)
        rows = torch.cat((self._buf[self.n - ctx:self.n], new)) if ctx > 0 else new
        return self.eng.score_seq_above(rows, self.pooled, int(seq_len), threshold, window=window, row0=self.n - ctx,
                                        causal=causal, context=ctx, reverse=reverse)

    def query_ids_seq_above(self, first, count, seq_len, threshold, window=-1, causal=False, reverse="both"):
        """Every member whose sequence-matched score is >= threshold for the run of members first .. first + count - 1
        (rows counted from `first`), the up to seq_len - 1 members before it serving as context rows."""
        self._no_sessions("query_ids_seq_above")
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.n:
            raise IndexError("query_ids_seq_above: first .. first + count must lie in [0, %d]" % self.n)
        ctx = min(int(seq_len) - 1, first)
        return self.eng.score_seq_above(self._buf[first - ctx:first + count], self.pooled, int(seq_len), threshold,
                                        window=window, row0=first - ctx, causal=causal, context=ctx, reverse=reverse)

    def query_closures(self, centers, labels, threshold, seq_len=1, slopes=None, min_terms=1, window=-1, causal=False,
                       reverse="both", pooled=None):
        """Every member that new scans (NOT in the database: frames len(db), len(db) + 1, ... of the current session,
        or, pooled=, their embedded vectors) are a closure of, on a map of any number of sessions
        (engine.Engine.score_session_above): the session-aware path-set score - sums and the window stop at session
        seams - folded over the candidates with at least `min_terms` terms, >= threshold.  The context rows are the up
        to seq_len - 1 last members of the current session, as in query_seq; slopes as there (None: the unit path).
        -> (rows i32 [n], ids i32 [n], scores f32 [n], codes u8 [n]: direction bit | path << 1, row_ptr i64 [g+1]).
        Fed one scan at a time it returns the pairs of one offline query_ids_closures call, under query_seq's
        condition (causal, window >= the paths' largest offset)."""
        new = self._embed(centers, labels) if pooled is None else self.eng._pooled(pooled, "pooled")
        ctx = min(int(seq_len) - 1, self.n - self._starts[-1])
        rows = torch.cat((self._buf[self.n - ctx:self.n], new)) if ctx > 0 else new
        return self.eng.score_session_above(rows, self.pooled, int(seq_len), threshold,
                                            None if slopes is None else self._paths(seq_len, slopes),
                                            col_sessions=self.session_starts, min_terms=int(min_terms), window=window,
                                            row0=self.n - ctx, causal=causal, context=ctx, reverse=reverse)

    def query_ids_closures(self, first, count, threshold, seq_len=1, slopes=None, min_terms=1, window=-1, causal=False,
                           reverse="both"):
        """query_closures for the run of members first .. first + count - 1 (their ids are their frames; rows counted
        from `first`), the up to seq_len - 1 members before `first` serving as context rows; sums stop at the session
        seams among them."""
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.n:
            raise IndexError("query_ids_closures: first .. first + count must lie in [0, %d]" % self.n)
        ctx = min(int(seq_len) - 1, first)
        return self.eng.score_session_above(self._buf[first - ctx:first + count], self.pooled, int(seq_len), threshold,
                                            None if slopes is None else self._paths(seq_len, slopes),
                                            row_sessions=self._session_rows(first - ctx, ctx + count),
                                            col_sessions=self.session_starts, min_terms=int(min_terms), window=window,
                                            row0=first - ctx, causal=causal, context=ctx, reverse=reverse)

    def save(self, path):
        dims = np.array([getattr(self.eng.dims, f) for f in _DIMS], dtype=np.int64)
        extra = {"session_starts": self.session_starts} if self._multi else {}
        np.savez(path, pooled=self.pooled.cpu().numpy(), dims=dims, weights_sha256=np.array(weights_sha256(self.model)),
                 **extra)

    @classmethod
    def load(cls, path, model):
        with np.load(path, allow_pickle=False) as z:
            pooled, dims, sha = z["pooled"], z["dims"], str(z["weights_sha256"])
            starts = z["session_starts"] if "session_starts" in z.files else None
        if sha != weights_sha256(model):
            raise ValueError("%s was built with another checkpoint (weights sha256 %s...)" % (path, sha[:12]))
        db = cls(model, capacity=max(pooled.shape[0], 1))
        have = np.array([getattr(db.eng.dims, f) for f in _DIMS], dtype=np.int64)
        if not np.array_equal(have, dims) or pooled.shape[1] != db.eng.pw:
            raise ValueError("%s holds vectors of another architecture (dims %s)" % (path, dims.tolist()))
        db.append_pooled(torch.from_numpy(pooled))
        if starts is not None:
            starts = [int(v) for v in starts]
            if (not starts or starts[0] != 0 or any(b <= a for a, b in zip(starts, starts[1:])) or starts[-1] > db.n
                    or len(starts) > _engine.SESSION_MAX):
                raise ValueError("%s holds a broken session table %s" % (path, starts))
            db._starts = starts
        return db


def main(argv=None):
    import sys
    from .graph_store import PackedSequence, pack_directory
    from .parser_sg import sgpr_args
    from .sg_net import SGTrainer
    ap = argparse.ArgumentParser(prog="python -m sg_pr_amd.place_db")
    ap.add_argument("config", nargs="?", default="./config/config.yml")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--causal", action="store_true")
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--hard", type=int, default=None, metavar="K",
                    help="also write <seq>_hard.npz: every frame's K hardest negatives and positives (1..16)")
    ap.add_argument("--recall-percent", type=float, default=None, metavar="P",
                    help="also report recall@P%% (N = max(1, round(frames * P / 100)) candidates, k = max(--k, N))")
    ap.add_argument("--seq-len", type=int, default=1, metavar="L",
                    help="rank the sequence-matched score: the mean along the last L frames of both trajectories (1..32)")
    ap.add_argument("--seq-reverse", choices=("off", "on", "both"), default="both",
                    help="with --seq-len: forward diagonals only (off), reverse only (on) or the larger of both")
    ap.add_argument("--verify", action="store_true",
                    help="verify the retrieved lists geometrically, re-rank them by inliers and write <seq>_verify.npz")
    ap.add_argument("--min-inliers", type=int, default=12, metavar="I",
                    help="with --verify: accept a closure with at least I refined inliers")
    ap.add_argument("--consistent", action="store_true",
                    help="with --verify: keep the accepted closures that agree pair by pair through the poses "
                         "(with --sessions N: within each pair of sessions) and write <seq>_consistent.npz")
    ap.add_argument("--optimize", action="store_true",
                    help="with --consistent: relax the planar pose graph of the map over the consistent closures "
                         "(DESIGN.md §25) and print the trajectory error before and after")
    ap.add_argument("--align", action="store_true",
                    help="with --landmarks: align every scan to the landmark map (DESIGN.md §31) from its localised pose "
                         "(--localize) or the pose the map was built on, and write <seq>_align.npz; the map contains the "
                         "scan being aligned")
    ap.add_argument("--align-radii", default="2,0.75", metavar="R,R,..",
                    help="with --align or --update: the gate schedule in metres, one call per gate")
    ap.add_argument("--align-iters", type=int, default=10, metavar="T",
                    help="with --align or --update: association and fit rounds per gate")
    ap.add_argument("--update", action="store_true",
                    help="with --landmarks --sessions N: build the landmark map on every session but the last, align the "
                         "last session to it and fold it in (DESIGN.md §32); writes <seq>_update.npz")
    ap.add_argument("--track", action="store_true",
                    help="with --landmarks --sessions N: track the last session through the landmark map of the others from "
                         "one initial pose (DESIGN.md §34); writes <seq>_track.npz")
    ap.add_argument("--track-radii", default="2,0.75", metavar="R,R,..",
                    help="with --track: the gates every scan runs, metres, wide to narrow")
    ap.add_argument("--reacquire-radii", default="8", metavar="R,..",
                    help="with --track: the gates run in front of them on the scan after a lost one (empty: none)")
    ap.add_argument("--min-matched", type=int, default=10, metavar="M",
                    help="with --track: a scan with fewer matches is lost and keeps its predicted pose")
    ap.add_argument("--relocalize", action="store_true",
                    help="with --landmarks --sessions N: relocalise every scan of the last session in the landmark map of the "
                         "others with no prior pose (DESIGN.md §35); writes <seq>_relocalize.npz")
    ap.add_argument("--reloc-min-inliers", type=int, default=12, metavar="I",
                    help="with --relocalize: a scan is found when its best pose puts that many nodes on landmarks")
    ap.add_argument("--reloc-max-base", type=float, default=30.0, metavar="B",
                    help="with --relocalize: the largest distance of the two nodes of a hypothesis, metres")
    ap.add_argument("--reloc-sep", type=float, default=10.0, metavar="S",
                    help="with --relocalize: how far from the answer another place is, metres")
    ap.add_argument("--retire", action="store_true",
                    help="with --update: tally what the drive folded in should have seen of the updated map and what it saw, "
                         "and retire the landmarks it should have seen and did not (DESIGN.md §33); writes <seq>_persist.npz. "
                         "There is no occlusion model: a hidden landmark counts as missed")
    ap.add_argument("--compact", action="store_true",
                    help="with --update [--retire]: compact the updated map on its records alone - drop what --retire "
                         "retired, fuse duplicates within --lm-radius, renumber (DESIGN.md §36); writes <seq>_compact.npz")
    ap.add_argument("--merge-maps", action="store_true",
                    help="with --landmarks --sessions N: build one landmark map per session and merge them left to right "
                         "on their records alone (DESIGN.md §36); writes <seq>_merge.npz")
    ap.add_argument("--view-range", type=float, default=50.0, metavar="R",
                    help="with --retire: the sensor range in metres; a scan sees as far as its farthest node, at most R")
    ap.add_argument("--view-margin", type=float, default=2.0, metavar="M",
                    help="with --retire: metres taken off a scan's range")
    ap.add_argument("--min-expected", type=int, default=5, metavar="E",
                    help="with --retire: a landmark is judged when at least E scans should have seen it")
    ap.add_argument("--max-seen-ratio", type=float, default=0.3, metavar="r",
                    help="with --retire: ... and retired when fewer than r of them did (0..1)")
    ap.add_argument("--save-poses", default=None, metavar="FILE",
                    help="with --optimize: write the optimised planar poses [M,4] (c, s, x, y) to FILE (.npy)")
    ap.add_argument("--localize", action="store_true",
                    help="with --verify: localise every scan in the sequence's poses from its verified candidates "
                         "(DESIGN.md §26) and write <seq>_localize.npz")
    ap.add_argument("--loc-len", type=int, default=1, metavar="L",
                    help="with --localize: the candidates of the last L scans vote, carried forward by the odometry (1..16)")
    ap.add_argument("--min-support", type=int, default=3, metavar="S",
                    help="with --localize: a scan is localised when S hypotheses agree")
    ap.add_argument("--loc-max-trans", type=float, default=1.0, metavar="M",
                    help="with --localize: translation tolerance of two hypotheses, metres")
    ap.add_argument("--loc-max-yaw-deg", type=float, default=math.degrees(0.1), metavar="D",
                    help="with --localize: yaw tolerance of two hypotheses, degrees")
    ap.add_argument("--landmarks", action="store_true",
                    help="fuse the nodes of every scan into a landmark map (DESIGN.md §27) on the poses the run ends "
                         "with - the optimised ones after --optimize - and write <seq>_landmarks.npz")
    ap.add_argument("--lm-radius", type=float, default=0.75, metavar="R",
                    help="with --landmarks: nodes of one label within R metres of one another are one landmark")
    ap.add_argument("--lm-tau-z", type=float, default=0.75, metavar="Z",
                    help="with --landmarks: ... and within Z metres in height")
    ap.add_argument("--lm-min-sessions", type=int, default=1, metavar="S",
                    help="with --landmarks: report the landmarks seen by at least S sessions as kept (1..64)")
    ap.add_argument("--refine", action="store_true",
                    help="with --landmarks: refine the poses the run ends with on the map's own landmarks (DESIGN.md "
                         "§29) before the landmark map is written; --save-poses then gets the refined poses")
    ap.add_argument("--refine-rounds", type=int, default=2, metavar="R",
                    help="with --refine: rounds of (landmark map, select, refine)")
    ap.add_argument("--refine-iters", type=int, default=10, metavar="T",
                    help="with --refine: alternations of centre means and pose fits per round")
    ap.add_argument("--max-trans", type=float, default=1.0, metavar="M",
                    help="with --consistent: translation tolerance of a pair of closures, metres")
    ap.add_argument("--max-yaw-deg", type=float, default=math.degrees(0.06), metavar="D",
                    help="with --consistent: yaw tolerance of a pair of closures, degrees")
    ap.add_argument("--lever-gain", type=float, default=0.04, metavar="G",
                    help="with --consistent: extra translation tolerance per metre between the two row scans")
    ap.add_argument("--min-clique", type=int, default=3, metavar="N",
                    help="with --consistent: a group whose consistent set is smaller than N accepts nothing")
    ap.add_argument("--distinct", type=int, default=None, metavar="RHO",
                    help="also retrieve the K best distinct places: score peaks within RHO frames (0..1024)")
    ap.add_argument("--seq-slopes", default=None, metavar="S,S,...",
                    help="with --seq-len: also retrieve the lists of the best mean over paths of these slopes, e.g. "
                         "1,1/2,2/3,3/2,2; writes <seq>_slopes.npz")
    ap.add_argument("--sessions", type=int, default=None, metavar="N",
                    help="also retrieve with the sequence split into N consecutive sessions (2..%d); writes "
                         "<seq>_sessions.npz" % _engine.SESSION_MAX)
    ap.add_argument("--min-terms", type=int, default=None, metavar="K",
                    help="with --threshold and --sessions or --seq-slopes: a path mean counts only with at least K terms "
                         "(1..--seq-len; default 1)")
    opt = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if opt.min_terms is not None and opt.threshold is None:
        ap.error("--min-terms needs --threshold")
    if opt.min_terms is not None and not 1 <= opt.min_terms <= max(opt.seq_len, 1):
        ap.error("--min-terms must lie in 1..--seq-len")
    if opt.consistent and not opt.verify:
        ap.error("--consistent needs --verify")
    if opt.optimize and not opt.consistent:
        ap.error("--optimize needs --consistent")
    if opt.refine and not opt.landmarks:
        ap.error("--refine needs --landmarks")
    if opt.refine and not (opt.refine_rounds >= 1 and opt.refine_iters >= 0):
        ap.error("--refine-rounds must be >= 1, --refine-iters >= 0")
    if opt.align and not opt.landmarks:
        ap.error("--align needs --landmarks")
    if opt.update and not (opt.landmarks and opt.sessions is not None):
        ap.error("--update needs --landmarks and --sessions N")
    if opt.retire and not opt.update:
        ap.error("--retire needs --update")
    if opt.compact and not opt.update:
        ap.error("--compact needs --update")
    if opt.merge_maps and not (opt.landmarks and opt.sessions is not None):
        ap.error("--merge-maps needs --landmarks and --sessions N")
    if opt.track:
        if not (opt.landmarks and opt.sessions is not None):
            ap.error("--track needs --landmarks and --sessions N")
        try:
            opt.track_radii = [float(t) for t in opt.track_radii.split(",") if t.strip()]
            opt.reacquire_radii = [float(t) for t in opt.reacquire_radii.split(",") if t.strip()]
        except ValueError:
            ap.error("--track-radii and --reacquire-radii are comma-separated lists of metres")
        from .landmarks import TRACK_MAX_STAGES
        if not (opt.track_radii and all(r > 0 for r in opt.track_radii + opt.reacquire_radii)
                and len(opt.track_radii) + len(opt.reacquire_radii) <= TRACK_MAX_STAGES and opt.min_matched >= 0
                and opt.align_iters >= 0):
            ap.error("--track-radii and --reacquire-radii must be positive, at most %d gates together; --min-matched and "
                     "--align-iters >= 0" % TRACK_MAX_STAGES)
    if opt.relocalize:
        if not (opt.landmarks and opt.sessions is not None):
            ap.error("--relocalize needs --landmarks and --sessions N")
        if not (opt.reloc_min_inliers >= 2 and 5.0 <= opt.reloc_max_base < math.inf and opt.reloc_sep >= 0):
            ap.error("--reloc-min-inliers must be >= 2, --reloc-max-base a finite number of metres >= 5, --reloc-sep >= 0")
    if opt.retire and not (opt.view_range >= 0 and 0 <= opt.view_margin < math.inf and opt.min_expected >= 0
                           and 0 <= opt.max_seen_ratio <= 1):
        ap.error("--view-range, --view-margin and --min-expected must be >= 0, --max-seen-ratio in 0..1")
    if opt.align or opt.update or opt.relocalize:
        try:
            opt.align_radii = [float(t) for t in opt.align_radii.split(",") if t.strip()]
        except ValueError:
            ap.error("--align-radii is a comma-separated list of metres")
        if not (opt.align_radii and all(r > 0 for r in opt.align_radii) and opt.align_iters >= 0):
            ap.error("--align-radii must be positive, --align-iters >= 0")
    if opt.save_poses is not None and not (opt.optimize or opt.refine):
        ap.error("--save-poses needs --optimize")
    if opt.consistent and (opt.max_trans < 0 or opt.lever_gain < 0 or not 0 <= opt.max_yaw_deg <= 180):
        ap.error("--max-trans and --lever-gain must be >= 0, --max-yaw-deg in 0..180")
    if opt.landmarks and not (opt.lm_radius > 0 and opt.lm_tau_z >= 0 and 1 <= opt.lm_min_sessions <= _engine.SESSION_MAX):
        ap.error("--lm-radius must be > 0, --lm-tau-z >= 0, --lm-min-sessions in 1..%d" % _engine.SESSION_MAX)
    if opt.localize and not opt.verify:
        ap.error("--localize needs --verify")
    from .localize import MAX_LEN as loc_max_len
    if opt.localize and not (1 <= opt.loc_len <= loc_max_len and opt.loc_max_trans >= 0 and 0 <= opt.loc_max_yaw_deg <= 180):
        ap.error("--loc-len must lie in 1..%d, --loc-max-trans must be >= 0, --loc-max-yaw-deg in 0..180" % loc_max_len)
    if opt.sessions is not None and not 2 <= opt.sessions <= _engine.SESSION_MAX:
        ap.error("--sessions must lie in 2..%d" % _engine.SESSION_MAX)
    if opt.sessions is not None and opt.distinct is not None:
        ap.error("--sessions does not compose with --distinct")
    paths = None
    if opt.seq_slopes is not None:
        if opt.seq_len < 2:
            ap.error("--seq-slopes needs --seq-len L > 1")
        try:
            slopes = [t for t in opt.seq_slopes.split(",") if t.strip()]
            paths = _engine.seq_paths(opt.seq_len, slopes)
        except (ValueError, ZeroDivisionError) as e:
            ap.error("--seq-slopes: %s" % e)
    if opt.distinct is not None and not 0 <= opt.distinct <= _engine.Engine.PEAK_MAX_RADIUS:
        ap.error("--distinct must lie in 0..%d" % _engine.Engine.PEAK_MAX_RADIUS)
    if not 1 <= opt.seq_len <= _engine.Engine.SEQ_MAX_LEN:
        ap.error("--seq-len must lie in 1..%d" % _engine.Engine.SEQ_MAX_LEN)
    args = sgpr_args()
    args.load(opt.config)
    trainer = SGTrainer(args, False)
    trainer.model.eval()
    os.makedirs(args.output_path, exist_ok=True)
    results = {}
    for sequence in args.sequences:
        cache = os.path.join(args.output_path, sequence + "_packed.npz")
        if os.path.exists(cache):
            seq = PackedSequence.load(cache)
        else:
            seq = pack_directory(os.path.join(args.graph_pairs_dir, sequence), int(args.node_num),
                                 trainer.number_of_labels)
            seq.save(cache)
        db = PlaceDatabase(trainer.model, capacity=len(seq))
        db.add(seq.centers, seq.labels)                    # the launch evaluate_all_pairs makes: size_order + ordered embed
        m = len(seq)
        k = opt.k
        extra = {}
        if opt.recall_percent is not None:
            k = max(k, metrics.recall_percent_n(m, opt.recall_percent))
        if opt.seq_len > 1:
            vals, idx, dirs = db.query_ids_seq(0, m, opt.seq_len, k=k, window=opt.window, causal=opt.causal,
                                               reverse={"off": False, "on": True, "both": "both"}[opt.seq_reverse])
            extra = {"seq_len": np.int64(opt.seq_len), "dirs": dirs.cpu().numpy()}
        else:
            vals, idx = db.query_ids(torch.arange(m), k=k, window=opt.window, causal=opt.causal)
        recall = metrics.recall_at_n(idx, seq.poses, p_thresh=float(args.p_thresh), window=opt.window, causal=opt.causal)
        if opt.recall_percent is not None:
            rp, n = metrics.recall_at_percent(idx, seq.poses, percent=opt.recall_percent, p_thresh=float(args.p_thresh),
                                              window=opt.window, causal=opt.causal)
            extra.update({"recall_percent": np.float64(rp), "recall_percent_n": np.int64(n)})
        np.savez(os.path.join(args.output_path, sequence + "_topk.npz"), frame=np.arange(m),
                 indices=idx.cpu().numpy(), scores=vals.cpu().numpy(), recall=recall, **extra)
        print("sequence", sequence, "frames", m, "recall@1..%d" % k, " ".join("%.4f" % r for r in recall))
        if opt.recall_percent is not None:
            print("sequence", sequence, "recall@%g%% (N = %d) %.4f" % (opt.recall_percent, extra["recall_percent_n"],
                                                                       extra["recall_percent"]))
        results[sequence] = recall
        if opt.verify:
            report = verify_lists(trainer.model, seq, vals, idx, opt.min_inliers, float(args.p_thresh), window=opt.window,
                                  causal=opt.causal)
            np.savez(os.path.join(args.output_path, sequence + "_verify.npz"), frame=np.arange(m), **report)
            print("sequence", sequence, "verified", int(report["verified"]), "candidates, recall@1 %.4f -> %.4f re-ranked,"
                  % (recall[0], report["recall_ranked"][0]), "accepted", int(report["accept"].sum()),
                  "(>= %d inliers) precision %.4f," % (opt.min_inliers, report["precision"]),
                  "accepted true closures %d: median yaw error %.3f deg, median translation error %.3f m"
                  % (int(report["true_accepted"]), report["median_yaw_deg"], report["median_trans_m"]))
        if opt.consistent:
            creport = consistent_lists(trainer.model, seq, vals, idx, opt.min_inliers, float(args.p_thresh),
                                       window=opt.window, causal=opt.causal, sessions=opt.sessions,
                                       max_trans=opt.max_trans, max_yaw=math.radians(opt.max_yaw_deg),
                                       lever_gain=opt.lever_gain, min_clique=opt.min_clique)
            np.savez(os.path.join(args.output_path, sequence + "_consistent.npz"), **creport)
            print("sequence", sequence, "sessions", opt.sessions or 1, "accepted", int(creport["accepted"]),
                  "precision %.4f" % creport["precision_accepted"], "-> pairwise consistent",
                  int(creport["consistent_count"]), "precision %.4f" % creport["precision_consistent"],
                  "(largest set %d)" % int(creport["group_size"].max()))
        if opt.optimize:
            X = metrics.planar_odometry(seq.poses)
            sel = {"accept": creport["consistent"]}
            out, info = trainer.model.optimize_map(sel, {"refined": creport["refined"]}, creport["rows"], creport["cols"], X,
                                                   sessions=creport["session_starts"])
            out = out.cpu().numpy()
            print("sequence", sequence, "pose graph over", info["live_closures"], "closures,", info["free_scans"],
                  "free scans in", info["active_sessions"], "sessions: trajectory error %.4f m -> %.4f m,"
                  % (metrics.trajectory_error(X, X), metrics.trajectory_error(out, X)),
                  "iterations %d + %d (%s, %s)" % (info["iterations"] + info["stop"]))
            if opt.save_poses is not None:
                with open(opt.save_poses, "wb") as f:
                    np.save(f, out)
        if opt.landmarks:
            starts = creport["session_starts"] if opt.consistent else None
            if opt.refine:
                rreport = refine_lists(trainer.model, seq, out if opt.optimize else None, sessions=starts,
                                       rounds=opt.refine_rounds, iters=opt.refine_iters, radius=opt.lm_radius,
                                       tau_z=opt.lm_tau_z)
                out = rreport["poses"]
                print("sequence", sequence, "refined on its landmarks, %d x %d iterations:" % (opt.refine_rounds, opt.refine_iters),
                      "landmarks %d -> %d, sharpness %.4f m -> %.4f m, shared %.4f -> %.4f,"
                      % tuple(rreport[a + n] for n in ("landmarks", "sharpness", "shared") for a in ("before_", "")),
                      "trajectory error %.4f m -> %.4f m," % (rreport["before_trajectory_error"], rreport["trajectory_error"]),
                      "%d of %d scans re-fitted" % (int(rreport["refitted"]), m))
                if opt.save_poses is not None:
                    with open(opt.save_poses, "wb") as f:
                        np.save(f, out)
            mreport = landmark_lists(trainer.model, seq, out if opt.optimize or opt.refine else None, sessions=starts,
                                     before=opt.optimize, radius=opt.lm_radius, tau_z=opt.lm_tau_z,
                                     min_sessions=opt.lm_min_sessions)
            np.savez(os.path.join(args.output_path, sequence + "_landmarks.npz"), **mreport)
            line = "landmarks %d sharpness %.4f m shared %.4f single %.4f" % tuple(
                mreport[n] for n in ("landmarks", "sharpness", "shared", "single"))
            if opt.optimize:
                line += " (before optimisation: landmarks %d sharpness %.4f m shared %.4f single %.4f)" % tuple(
                    mreport["before_" + n] for n in ("landmarks", "sharpness", "shared", "single"))
            print("sequence", sequence, "landmark map of", int(mreport["live_nodes"]), "nodes:", line + ",",
                  int(mreport["keep"].sum()), "seen by >= %d sessions" % opt.lm_min_sessions)
        if opt.localize:
            lreport = localize_lists(trainer.model, seq, vals, idx, opt.min_inliers, seq_len=opt.loc_len,
                                     min_support=opt.min_support, max_trans=opt.loc_max_trans,
                                     max_yaw=math.radians(opt.loc_max_yaw_deg))
            np.savez(os.path.join(args.output_path, sequence + "_localize.npz"), frame=np.arange(m), **lreport)
            print("sequence", sequence, "localised %.4f of %d scans (last %d scans, support >= %d):"
                  % (lreport["localized"], m, opt.loc_len, opt.min_support),
                  "translation error median %.3f m, 95%% %.3f m; yaw error median %.3f deg, 95%% %.3f deg;"
                  % tuple(lreport[n] for n in ("median_trans_m", "p95_trans_m", "median_yaw_deg", "p95_yaw_deg")),
                  "best verified candidate alone: %.4f, median %.3f m, 95%% %.3f m; median %.3f deg, 95%% %.3f deg"
                  % tuple(lreport["single_" + n] for n in ("localized", "median_trans_m", "p95_trans_m", "median_yaw_deg",
                                                           "p95_yaw_deg")))
        if opt.align:
            areport = align_lists(trainer.model, seq, mreport, located=lreport if opt.localize else None,
                                  radii=opt.align_radii, iters=opt.align_iters, tau_z=opt.lm_tau_z)
            np.savez(os.path.join(args.output_path, sequence + "_align.npz"), frame=np.arange(m), **areport)
            print("sequence", sequence, "aligned to its landmark map (which contains the scans), gates %s m x %d iterations:"
                  % (", ".join("%g" % r for r in opt.align_radii), opt.align_iters),
                  "translation %.4f / %.4f m -> %.4f / %.4f m (median / 95%%), yaw %.4f / %.4f deg -> %.4f / %.4f deg,"
                  % tuple(areport[a + n] for n in ("trans_m", "yaw_deg") for a in ("before_median_", "before_p95_", "median_", "p95_")),
                  "matched share %.4f (median), unmatched live nodes %d, accepted %d of %d, started from a localised pose %d"
                  % (areport["matched_share"], int(areport["unmatched"]), int(areport["accept"].sum()), m,
                     int(areport["from_localize"].sum())))
        if opt.update:
            ureport = update_lists(trainer.model, seq, opt.sessions, radii=opt.align_radii, iters=opt.align_iters,
                                   radius=opt.lm_radius, tau_z=opt.lm_tau_z)
            np.savez(os.path.join(args.output_path, sequence + "_update.npz"), **ureport)
            print("sequence", sequence, "session %d of %d folded into the landmark map of the others, gates %s m x %d iterations:"
                  % (int(ureport["session"]), opt.sessions, ", ".join("%g" % r for r in opt.align_radii), opt.align_iters),
                  "landmarks %d -> %d (%d new), observed nodes %d, new nodes %d,"
                  % (int(ureport["landmarks_before"]), int(ureport["num"][0]), int(ureport["num"][0] - ureport["landmarks_before"]),
                     int(ureport["num"][2]), int(ureport["num"][3])),
                  "count as in the batch map of %d landmarks: %.4f" % (int(ureport["batch_landmarks"]), ureport["same_count"]))
            if opt.retire:
                preport = persist_lists(trainer.model, seq, ureport, max_range=opt.view_range, margin=opt.view_margin,
                                        min_expected=opt.min_expected, max_seen_ratio=opt.max_seen_ratio, radius=opt.lm_radius)
                np.savez(os.path.join(args.output_path, sequence + "_persist.npz"), **preport)
                print("sequence", sequence, "session %d tallied on the updated map (view %g m less %g m, no occlusion model):"
                      % (int(ureport["session"]), opt.view_range, opt.view_margin),
                      "landmarks in use %d -> %d, retired %d of %d judged (expected >= %d, seen < %g of expected),"
                      % (int(preport["in_use_before"]), int(preport["in_use_after"]), int(preport["num"][0]), int(preport["num"][1]),
                         opt.min_expected, opt.max_seen_ratio),
                      "per-scan seen / expected %.4f (median)" % preport["scan_ratio_median"])
            if opt.compact:
                kreport = compact_lists(trainer.model, ureport, keep=preport["keep"] if opt.retire else None,
                                        radius=opt.lm_radius, tau_z=opt.lm_tau_z)
                np.savez(os.path.join(args.output_path, sequence + "_compact.npz"), **kreport)
                print("sequence", sequence, "updated map compacted on its records (%s, radius %g m):"
                      % ("under the retire mask" if opt.retire else "no mask", opt.lm_radius),
                      "landmarks %d -> %d, dropped %d, fused %d"
                      % (int(kreport["landmarks_before"]), int(kreport["num"][0]), int(kreport["num"][1] + kreport["num"][2]),
                         int(kreport["num"][3])))
        if opt.merge_maps:
            greport = merge_lists(trainer.model, seq, opt.sessions, radius=opt.lm_radius, tau_z=opt.lm_tau_z)
            np.savez(os.path.join(args.output_path, sequence + "_merge.npz"), **greport)
            print("sequence", sequence, "landmark maps of %d sessions merged on their records (radius %g m):" % (opt.sessions, opt.lm_radius),
                  "landmarks %s -> %d, fused %d; the batch map of every session has %d landmarks, count as in it: %.4f"
                  % (" + ".join(str(int(v)) for v in greport["landmarks_per_session"]), int(greport["num"][0]),
                     int(greport["fused"].sum()), int(greport["batch_landmarks"]), greport["same_count"]))
        rreport = None
        if opt.relocalize:
            rreport = relocalize_lists(trainer.model, seq, opt.sessions, radii=opt.align_radii, iters=opt.align_iters,
                                       min_inliers=opt.reloc_min_inliers, max_base=opt.reloc_max_base, sep=opt.reloc_sep,
                                       radius=opt.lm_radius, tau_z=opt.lm_tau_z)
            np.savez(os.path.join(args.output_path, sequence + "_relocalize.npz"), **rreport)
            print("sequence", sequence, "session %d of %d relocalised in the landmark map of the others with no prior pose, base "
                  "pairs up to %g m, %d inliers, gates %s m x %d iterations:"
                  % (int(rreport["session"]), opt.sessions, opt.reloc_max_base, opt.reloc_min_inliers,
                     ", ".join("%g" % r for r in opt.align_radii), opt.align_iters),
                  "found %.4f, ambiguous %.4f of %d scans (another place beyond %g m with 0.7 of the inliers),"
                  % (rreport["found"].mean() if rreport["found"].size else 0.0,
                     rreport["ambiguous"].mean() if rreport["found"].size else 0.0, rreport["found"].shape[0], opt.reloc_sep),
                  "translation of the found %.4f / %.4f m (median / max), hypotheses %d / %d (median / max)"
                  % (rreport["median_trans_m"], rreport["max_trans_m"], int(np.median(rreport["hypotheses"])) if
                     rreport["found"].size else 0, int(rreport["hypotheses"].max()) if rreport["found"].size else 0))
        if opt.track:
            seed = None
            if rreport is not None and not opt.localize:
                seed = relocalized_start(rreport, seq.labels.shape[0])
            treport = track_lists(trainer.model, seq, opt.sessions, located=lreport if opt.localize else seed,
                                  radii=opt.track_radii, reacquire_radii=opt.reacquire_radii, iters=opt.align_iters,
                                  min_matched=opt.min_matched, radius=opt.lm_radius, tau_z=opt.lm_tau_z)
            np.savez(os.path.join(args.output_path, sequence + "_track.npz"), **treport)
            print("sequence", sequence, "session %d of %d tracked through the landmark map of the others, gates %s m (after a lost "
                  "scan %s m first) x %d iterations:"
                  % (int(treport["session"]), opt.sessions, ", ".join("%g" % r for r in opt.track_radii),
                     ", ".join("%g" % r for r in opt.reacquire_radii) or "-", opt.align_iters),
                  "tracked %d, lost %d of %d scans (fewer than %d matches), longest lost run %d, matched share %.4f (median),"
                  % (int(treport["num"][0]), int(treport["num"][1]), treport["lost"].shape[0], opt.min_matched,
                     int(treport["num"][2]), treport["matched_share"]),
                  "translation %.4f / %.4f m (median / 95%%), first pose from %s"
                  % (treport["median_trans_m"], treport["p95_trans_m"], ("relocalize" if rreport is not None and not opt.localize else "localize") if treport["from_localize"]
                     else "the stored pose"))
        if opt.distinct is not None:
            if opt.seq_len > 1:
                dvals, didx, ddirs = db.query_ids_seq(0, m, opt.seq_len, k=k, window=opt.window, causal=opt.causal,
                                                      reverse={"off": False, "on": True, "both": "both"}[opt.seq_reverse],
                                                      distinct=opt.distinct)
                dextra = {"seq_len": np.int64(opt.seq_len), "dirs": ddirs.cpu().numpy()}
            else:
                dvals, didx = db.query_ids(torch.arange(m), k=k, window=opt.window, causal=opt.causal,
                                           distinct=opt.distinct)
                dextra = {}
            drecall = metrics.recall_at_n(didx, seq.poses, p_thresh=float(args.p_thresh), window=opt.window,
                                          causal=opt.causal)
            np.savez(os.path.join(args.output_path, sequence + "_distinct.npz"), frame=np.arange(m),
                     indices=didx.cpu().numpy(), scores=dvals.cpu().numpy(), recall=drecall,
                     radius=np.int64(opt.distinct), **dextra)
            print("sequence", sequence, "distinct radius", opt.distinct, "recall@1 %.4f (plain %.4f)" % (drecall[0], recall[0]),
                  "recall@%d %.4f (plain %.4f)" % (k, drecall[-1], recall[-1]),
                  "places per list %.3f (plain %.3f)" % (metrics.places_per_list(didx, opt.distinct),
                                                         metrics.places_per_list(idx, opt.distinct)))
            if opt.verify:
                dreport = verify_lists(trainer.model, seq, dvals, didx, opt.min_inliers, float(args.p_thresh),
                                       window=opt.window, causal=opt.causal)
                np.savez(os.path.join(args.output_path, sequence + "_distinct_verify.npz"), frame=np.arange(m), **dreport)
                print("sequence", sequence, "pairs verified: plain", int(report["verified"]), "distinct",
                      int(dreport["verified"]), "recall@1 re-ranked %.4f (plain %.4f)"
                      % (dreport["recall_ranked"][0], report["recall_ranked"][0]))
        if paths is not None:
            svals, sidx, scodes = db.query_ids_seq(0, m, opt.seq_len, k=k, window=opt.window, causal=opt.causal,
                                                   reverse={"off": False, "on": True, "both": "both"}[opt.seq_reverse],
                                                   distinct=opt.distinct, slopes=slopes)
            srecall = metrics.recall_at_n(sidx, seq.poses, p_thresh=float(args.p_thresh), window=opt.window,
                                          causal=opt.causal)
            sextra = {} if opt.distinct is None else {"radius": np.int64(opt.distinct)}
            codes = scodes.cpu().numpy()
            np.savez(os.path.join(args.output_path, sequence + "_slopes.npz"), frame=np.arange(m),
                     indices=sidx.cpu().numpy(), scores=svals.cpu().numpy(), codes=codes, paths=paths, recall=srecall,
                     seq_len=np.int64(opt.seq_len), **sextra)
            listed = (sidx >= 0).cpu().numpy()
            share = np.bincount(codes[listed] >> 1, minlength=paths.shape[0]) / max(int(listed.sum()), 1)
            # the unit-slope lists beside them: the distinct ones when --distinct is given
            urecall = drecall if opt.distinct is not None else recall
            print("sequence", sequence, "slopes", opt.seq_slopes, "paths", paths.shape[0],
                  "recall@1 %.4f (unit slope %.4f)" % (srecall[0], urecall[0]),
                  "recall@%d %.4f (unit slope %.4f)" % (k, srecall[-1], urecall[-1]),
                  "share of listed entries per path", " ".join("%.3f" % x for x in share))
        if opt.sessions is not None:
            report = session_lists(db, seq.poses, opt.sessions, idx, k=k, window=opt.window, causal=opt.causal,
                                   seq_len=opt.seq_len, p_thresh=float(args.p_thresh),
                                   reverse={"off": False, "on": True, "both": "both"}[opt.seq_reverse],
                                   slopes=slopes if paths is not None else None)
            np.savez(os.path.join(args.output_path, sequence + "_sessions.npz"), frame=np.arange(m),
                     **report, **({"seq_len": np.int64(opt.seq_len)} if opt.seq_len > 1 else {}))
            for name, what in (("recall", "all rows"), ("recall_head", "head rows (%d)" % int(report["head_rows"]))):
                one = report[name + "_one_trajectory"]
                print("sequence", sequence, "sessions", opt.sessions, what,
                      "recall@1 %.4f (one trajectory %.4f)" % (report[name][0], one[0]),
                      "recall@%d %.4f (one trajectory %.4f)" % (k, report[name][-1], one[-1]))
        if opt.threshold is not None:
            rows, cols, scores, _ = db.query_ids_above(torch.arange(m), opt.threshold, window=opt.window,
                                                       causal=opt.causal)
            precision, rec = metrics.precision_recall_at(rows, cols, seq.poses, p_thresh=float(args.p_thresh),
                                                         window=opt.window, causal=opt.causal)
            np.savez(os.path.join(args.output_path, sequence + "_above.npz"), rows=rows.cpu().numpy(),
                     cols=cols.cpu().numpy(), scores=scores.cpu().numpy(), precision=precision, recall=rec)
            print("sequence", sequence, "threshold", opt.threshold, "pairs", rows.numel(),
                  "precision %.4f recall %.4f" % (precision, rec))
        if opt.threshold is not None and opt.seq_len > 1:
            rows, cols, scores, dirs, _ = db.query_ids_seq_above(
                0, m, opt.seq_len, opt.threshold, window=opt.window, causal=opt.causal,
                reverse={"off": False, "on": True, "both": "both"}[opt.seq_reverse])
            precision, rec = metrics.precision_recall_at(rows, cols, seq.poses, p_thresh=float(args.p_thresh),
                                                         window=opt.window, causal=opt.causal)
            np.savez(os.path.join(args.output_path, sequence + "_seq_above.npz"), rows=rows.cpu().numpy(),
                     cols=cols.cpu().numpy(), scores=scores.cpu().numpy(), dirs=dirs.cpu().numpy(), precision=precision,
                     recall=rec, seq_len=np.int64(opt.seq_len))
            print("sequence", sequence, "sequence length", opt.seq_len, "threshold", opt.threshold, "pairs", rows.numel(),
                  "precision %.4f recall %.4f" % (precision, rec))
        if opt.threshold is not None and (opt.sessions is not None or paths is not None):
            report = session_closures(db, seq.poses, opt.sessions or 1, opt.threshold, window=opt.window,
                                      causal=opt.causal, seq_len=opt.seq_len, p_thresh=float(args.p_thresh),
                                      reverse={"off": False, "on": True, "both": "both"}[opt.seq_reverse],
                                      slopes=slopes if paths is not None else None, min_terms=opt.min_terms or 1)
            np.savez(os.path.join(args.output_path, sequence + "_session_above.npz"), **report)
            print("sequence", sequence, "sessions", opt.sessions or 1, "sequence length", opt.seq_len, "min terms",
                  opt.min_terms or 1, "threshold", opt.threshold, "pairs", report["rows"].size,
                  "precision %.4f recall %.4f" % (report["precision"], report["recall"]))
        if opt.hard is not None:
            hard = hard_pairs_of(db, seq.poses, opt.hard, float(args.p_thresh), window=opt.window, causal=opt.causal)
            np.savez(os.path.join(args.output_path, sequence + "_hard.npz"), frame=np.arange(m), **hard)
            print("sequence", sequence, "hard pairs k", opt.hard, "frames with a negative above their best positive",
                  int(hard["neg_above_pos"].sum()), "(exact: %d frames of %d)" % (int(hard["exact"].sum()), m))
    return results


def session_lists(db, poses, sessions, one_idx, k=1, window=50, causal=False, seq_len=1, p_thresh=3.0, reverse="both",
                  slopes=None):
    """The members of `db` taken as `sessions` consecutive near-equal sessions (session j starts at (j * M) // sessions)
    and retrieved through the session call; one_idx: the one-trajectory lists to judge beside them -> dict of numpy
    arrays: indices, scores, codes, session_starts, recall / recall_head (head rows: fewer than `window` scans after
    the start of a session with a predecessor) and the same two of one_idx, all under the session rule, head_rows."""
    m = len(db)
    sdb = PlaceDatabase(db.model, capacity=max(m, 1))
    bounds = [(j * m) // int(sessions) for j in range(int(sessions))] + [m]
    for a, b in zip(bounds, bounds[1:]):
        sdb.new_session()
        sdb.append_pooled(db.pooled[a:b])
    starts = sdb.session_starts
    if seq_len > 1:
        vals, idx, codes = sdb.query_ids_seq(0, m, seq_len, k=k, window=window, causal=causal, reverse=reverse,
                                             slopes=slopes)
        codes = codes.cpu().numpy()
    else:
        vals, idx = sdb.query_ids(torch.arange(m), k=k, window=window, causal=causal)
        codes = np.zeros(tuple(idx.shape), dtype=np.uint8)
    frames = np.arange(m)
    head = np.zeros(m, dtype=bool)
    for s0 in starts[1:]:
        head |= (frames >= s0) & (frames < s0 + max(int(window), 0))
    kw = dict(p_thresh=p_thresh, window=window, causal=causal, col_starts=starts)
    return {"indices": idx.cpu().numpy(), "scores": vals.cpu().numpy(), "codes": codes, "session_starts": starts,
            "recall": metrics.recall_at_n(idx, poses, **kw),
            "recall_head": metrics.recall_at_n(idx, poses, row_mask=head, **kw),
            "recall_one_trajectory": metrics.recall_at_n(one_idx, poses, **kw),
            "recall_head_one_trajectory": metrics.recall_at_n(one_idx, poses, row_mask=head, **kw),
            "head_rows": np.int64(int(head.sum()))}


def session_closures(db, poses, sessions, threshold, window=50, causal=False, seq_len=1, p_thresh=3.0, reverse="both",
                     slopes=None, min_terms=1):
    """The members of `db` taken as `sessions` consecutive near-equal sessions (session_lists' split) and thresholded
    through PlaceDatabase.query_ids_closures -> dict of numpy arrays: rows, cols, scores, codes, row_ptr,
    session_starts, seq_len, min_terms, precision and recall (metrics.precision_recall_at under the session rule)."""
    m = len(db)
    sdb = PlaceDatabase(db.model, capacity=max(m, 1))
    bounds = [(j * m) // int(sessions) for j in range(int(sessions))] + [m]
    for a, b in zip(bounds, bounds[1:]):
        sdb.new_session()
        sdb.append_pooled(db.pooled[a:b])
    starts = sdb.session_starts
    rows, cols, scores, codes, row_ptr = sdb.query_ids_closures(0, m, threshold, seq_len=seq_len, slopes=slopes,
                                                                min_terms=min_terms, window=window, causal=causal,
                                                                reverse=reverse)
    precision, rec = metrics.precision_recall_at(rows, cols, poses, p_thresh=p_thresh, window=window, causal=causal,
                                                 col_starts=starts)
    return {"rows": rows.cpu().numpy(), "cols": cols.cpu().numpy(), "scores": scores.cpu().numpy(),
            "codes": codes.cpu().numpy(), "row_ptr": row_ptr.cpu().numpy(), "session_starts": starts,
            "seq_len": np.int64(seq_len), "min_terms": np.int64(min_terms), "precision": np.float64(precision),
            "recall": np.float64(rec)}


def verify_lists(model, seq, values, indices, min_inliers, p_thresh, window=-1, causal=False):
    """Geometric verification of retrieved lists (values / indices [M,K] of the frames of `seq` against themselves) ->
    dict of numpy arrays: the per-slot fields, indices_ranked, accept, recall_ranked [K] (recall@1..K of the re-ranked
    lists), precision of the accepted closures (metrics.precision_recall_at's classes), true_accepted = the accepted
    closures within p_thresh and the median yaw / translation error of those (metrics.closure_pose_errors; 0 when there
    is none)."""
    ver = model.verify_closures(seq.centers, seq.labels, indices, values=values, min_inliers=min_inliers)
    idx = torch.as_tensor(indices).to(ver["accept"].device)
    m, k = idx.shape
    rows = torch.arange(m, device=idx.device)[:, None].expand(m, k)
    acc = ver["accept"]
    arows, acols = rows[acc], idx[acc].long()
    precision = metrics.precision_recall_at(arows, acols, seq.poses, p_thresh=p_thresh, window=window, causal=causal)[0]
    err = metrics.closure_pose_errors({"refined": ver["refined"][acc], "flags": ver["flags"][acc]}, arows, acols, seq.poses)
    from .allpairs import pose_xz
    xz = pose_xz(seq.poses).to(device=idx.device, dtype=torch.float64)
    true = (((xz[arows] - xz[acols]) ** 2).sum(dim=1) <= p_thresh * p_thresh).cpu().numpy()
    yaw, trans = err["yaw_deg"][true], err["trans_m"][true]
    out = {name: ver[name].cpu().numpy() for name in ("inliers", "inliers_refined", "flags", "refined", "yaw", "rmse",
                                                      "indices_ranked", "accept")}
    out.update({"recall_ranked": metrics.recall_at_n(ver["indices_ranked"], seq.poses, p_thresh=p_thresh, window=window,
                                                     causal=causal),
                "verified": np.int64(int((idx >= 0).sum())), "precision": np.float64(precision),
                "true_accepted": np.int64(int(true.sum())),
                "median_yaw_deg": np.float64(np.median(yaw) if yaw.size else 0.0),
                "median_trans_m": np.float64(np.median(trans) if trans.size else 0.0)})
    return out


def localize_lists(model, seq, values, indices, min_inliers, seq_len=1, min_support=3, max_trans=1.0, max_yaw=0.1):
    """Every frame of `seq` localised in the sequence's own planar poses from the candidates its list retrieved (values /
    indices [M,K], at most localize.MAX_K columns of them): verified as verify_lists does, then SG.localize with the
    poses as the map and as the query drive's odometry.  Beside it the best verified candidate taken alone: the first
    slot of the re-ranked list, when it is accepted.
    -> dict of numpy arrays: pose [M,4], support, live, winner, flags, spread, accept (support >= min_support), trans_m,
    yaw_deg [M] (metrics.localization_errors against the poses; NaN where not accepted), localized (the share accepted),
    median / p95 of both errors over the accepted; single_pose, single_accept and the same five figures with the prefix
    single_; what went in: indices, refined, verify_flags, verify_accept, seq_len, min_support, max_trans, max_yaw."""
    from . import localize as _localize
    from .synth import _se2_compose
    idx = torch.as_tensor(indices)[:, :_localize.MAX_K]
    vals = None if values is None else torch.as_tensor(values)[:, :_localize.MAX_K]
    ver = model.verify_closures(seq.centers, seq.labels, idx, values=vals, min_inliers=min_inliers)
    X = metrics.planar_odometry(seq.poses)
    loc = model.localize(ver, idx, X, query_poses=X, seq_len=seq_len, min_support=min_support, max_trans=max_trans,
                         max_yaw=max_yaw)
    out = {name: loc[name].cpu().numpy() for name in ("pose", "support", "live", "winner", "flags", "spread", "accept")}
    idx_h, refined = idx.cpu().numpy(), ver["refined"].cpu().numpy()
    best = ver["order"][:, :1].cpu().numpy()
    single_ok = np.take_along_axis(ver["accept"].cpu().numpy(), best, axis=1)[:, 0]
    col = np.take_along_axis(idx_h, best, axis=1)[:, 0]
    single = _se2_compose(X[np.where(single_ok, col, 0)], np.take_along_axis(refined, best[:, :, None], axis=1)[:, 0])
    single[~single_ok] = np.nan

    def figures(pose, ok, prefix):
        err = metrics.localization_errors(np.where(ok[:, None], pose, np.nan), X)
        t, y = err["trans_m"][ok], err["yaw_deg"][ok]
        rep = {prefix + "localized": np.float64(ok.mean() if ok.size else 0.0)}
        for name, v in (("trans_m", t), ("yaw_deg", y)):
            rep[prefix + "median_" + name] = np.float64(np.median(v) if v.size else float("nan"))
            rep[prefix + "p95_" + name] = np.float64(np.percentile(v, 95) if v.size else float("nan"))
        return err, rep

    err, rep = figures(out["pose"], out["accept"], "")
    out.update(rep)
    out.update({"trans_m": err["trans_m"], "yaw_deg": err["yaw_deg"], "single_pose": single, "single_accept": single_ok})
    out.update(figures(single, single_ok, "single_")[1])
    out.update({"indices": idx_h, "refined": refined, "verify_flags": ver["flags"].cpu().numpy(),
                "verify_accept": ver["accept"].cpu().numpy(), "seq_len": np.int64(seq_len),
                "min_support": np.int64(min_support), "max_trans": np.float64(max_trans), "max_yaw": np.float64(max_yaw)})
    return out


def refine_lists(model, seq, poses=None, sessions=None, rounds=2, iters=10, radius=0.75, tau_z=0.75):
    """The planar `poses` [M,4] of `seq` - None: the sequence's own - refined on the map's landmarks (SG.refine_map) with
    `sessions` as the session table of its frames.
    -> dict: poses f64 [M,4] (numpy), cost [rounds, iters+1], refitted (scans the last fit moved), the figures landmarks,
    sharpness, shared (metrics.map_sharpness) and trajectory_error (metrics.trajectory_error against the sequence's own
    poses) of the refined map, and the same four with the prefix before_."""
    own = metrics.planar_odometry(seq.poses)
    X = own if poses is None else np.asarray(poses, dtype=np.float64).reshape(-1, 4)
    kw = dict(sessions=sessions, radius=radius, tau_z=tau_z)
    first = metrics.map_sharpness(model.landmark_map(seq.centers, seq.labels, X, **kw))
    Y, lm, costs = model.refine_map(seq.centers, seq.labels, X, rounds=rounds, iters=iters, **kw)
    Y = Y.cpu().numpy()
    out = {"poses": Y, "cost": np.stack(costs), "refitted": np.int64((Y != X).any(axis=1).sum()),
           "trajectory_error": metrics.trajectory_error(Y, own), "before_trajectory_error": metrics.trajectory_error(X, own)}
    last = metrics.map_sharpness(lm)
    out.update({n: last[n] for n in ("landmarks", "sharpness", "shared")})
    out.update({"before_" + n: first[n] for n in ("landmarks", "sharpness", "shared")})
    return out


def landmark_lists(model, seq, poses=None, sessions=None, before=False, radius=0.75, tau_z=0.75, min_sessions=1):
    """The landmark map of `seq` (SG.landmark_map) on planar `poses` [M,4] - None: the sequence's own - with `sessions`
    as the session table of its frames (None: one session).  before: also the figures of the map on the sequence's own
    poses, to set an optimised map against.
    -> dict of numpy arrays: center, label, count, first, sessions, spread per landmark, node_landmark [M,N], keep (the
    landmarks seen by at least min_sessions sessions), live_nodes, poses, radius, tau_z, min_sessions, the four figures of
    metrics.map_sharpness (landmarks, sharpness, shared, single) and, with before, the same four with the prefix before_."""
    from . import landmarks as _landmarks
    own = metrics.planar_odometry(seq.poses)
    X = own if poses is None else np.asarray(poses, dtype=np.float64).reshape(-1, 4)
    lm = model.landmark_map(seq.centers, seq.labels, X, sessions=sessions, radius=radius, tau_z=tau_z)
    out = {name: lm[name].cpu().numpy() for name in ("center", "label", "count", "first", "sessions", "spread",
                                                     "node_landmark")}
    out["keep"] = _landmarks.select(lm, min_sessions=min_sessions).cpu().numpy()
    out.update({"live_nodes": np.int64(lm["live_nodes"]), "poses": X, "radius": np.float64(radius),
                "tau_z": np.float64(tau_z), "min_sessions": np.int64(min_sessions)})
    out.update(metrics.map_sharpness(lm))
    if before:
        first = model.landmark_map(seq.centers, seq.labels, own, sessions=sessions, radius=radius, tau_z=tau_z)
        out.update({"before_" + k: v for k, v in metrics.map_sharpness(first).items()})
    return out


def align_lists(model, seq, lm, located=None, radii=(2.0, 0.75), iters=10, min_nodes=6, tau_z=0.75):
    """Every scan of `seq` aligned to the landmark map `lm` - the dict of landmark_lists: center, label, keep and the poses
    it was built on (SG.align_to_map).  located: the dict of localize_lists; its accepted scans start from its pose, every
    other scan from lm's.  The map contains the scans being aligned.
    -> dict: poses, start f64 [M,4], matched, live, steps, flags i32 [M], rms f64 [M], accept bool [M], node_landmark i32
    [M,N], from_localize bool [M], radii, iters, min_nodes; against the sequence's own poses (metrics.localization_errors)
    median_ / p95_ trans_m and yaw_deg with and without the prefix before_; matched_share (the median of matched / live
    over the scans with a live node), unmatched (the live nodes without a landmark)."""
    own = metrics.planar_odometry(seq.poses)
    start = np.array(np.asarray(lm["poses"], dtype=np.float64).reshape(-1, 4))
    given = np.zeros(start.shape[0], dtype=bool)
    if located is not None:
        given = np.asarray(located["accept"], dtype=bool).reshape(-1) & np.isfinite(located["pose"]).all(axis=1)
        start[given] = located["pose"][given]
    X, info = model.align_to_map(seq.centers, seq.labels, start, lm, keep=lm["keep"], radii=radii, iters=iters,
                                 min_nodes=min_nodes, tau_z=tau_z)
    X = X.cpu().numpy()
    out = {"poses": X, "start": start, "from_localize": given, "radii": np.asarray(radii, dtype=np.float64),
           "iters": np.int64(iters), "min_nodes": np.int64(min_nodes)}
    out.update({k: info[k] for k in ("matched", "live", "steps", "flags", "rms", "accept", "node_landmark")})
    for prefix, poses in (("before_", start), ("", X)):
        err = metrics.localization_errors(poses, own)
        for name in ("trans_m", "yaw_deg"):
            out[prefix + "median_" + name] = np.float64(np.median(err[name]))
            out[prefix + "p95_" + name] = np.float64(np.percentile(err[name], 95))
    seen = info["live"] > 0
    out["matched_share"] = np.float64(np.median(info["matched"][seen] / info["live"][seen]) if seen.any() else 0.0)
    out["unmatched"] = np.int64((info["node_landmark"] == -2).sum())
    return out


def update_lists(model, seq, sessions, radii=(2.0, 0.75), iters=10, min_nodes=6, radius=0.75, tau_z=0.75):
    """The last of `sessions` consecutive near-equal sessions of `seq` (session_lists' split) folded into the landmark map
    of the others: the map is built on the sequence's own poses (SG.landmark_map), the scans of the last session are
    aligned to all of its landmarks from their own poses (SG.align_to_map) and folded in (SG.update_map).  The yardstick
    is the batch map of every session on the same poses.
    -> dict of numpy arrays: center, label, count, first, sessions, spread of the updated map, node_landmark [Q,N] of the
    new scans, num = (landmarks, live, observed, new nodes), landmarks_before, batch_landmarks, same_count (the share of
    the updated landmarks whose count equals that of the batch landmark holding their first node), poses, start [Q,4],
    first_scan, session, node_base, radii, iters."""
    m, n = seq.labels.shape[0], seq.labels.shape[1]
    bounds = np.asarray([(j * m) // int(sessions) for j in range(int(sessions))], dtype=np.int32)
    b, last = int(bounds[-1]), int(sessions) - 1
    own = metrics.planar_odometry(seq.poses)
    lm = model.landmark_map(seq.centers[:b], seq.labels[:b], own[:b], sessions=bounds[:-1], radius=radius, tau_z=tau_z)
    X, _ = model.align_to_map(seq.centers[b:], seq.labels[b:], own[b:], lm, radii=radii, iters=iters, min_nodes=min_nodes,
                              tau_z=tau_z)
    up = model.update_map(seq.centers[b:], seq.labels[b:], X, lm, last, node_base=b * n, radius=radius, tau_z=tau_z)
    X = X.cpu().numpy()
    batch = model.landmark_map(seq.centers, seq.labels, np.concatenate((own[:b], X)), sessions=bounds, radius=radius,
                               tau_z=tau_z)
    out = {name: up[name].cpu().numpy() for name in ("center", "label", "count", "first", "sessions", "spread", "node_landmark")}
    holder = batch["node_landmark"].cpu().numpy().reshape(-1)[out["first"]]
    same = batch["count"].cpu().numpy()[holder] == out["count"]
    out.update({"num": np.asarray([up["num_landmarks"], up["live_nodes"], up["observed"], up["new_nodes"]], dtype=np.int64),
                "landmarks_before": np.int64(lm["num_landmarks"]), "batch_landmarks": np.int64(batch["num_landmarks"]),
                "same_count": np.float64(same.mean() if same.size else 1.0), "poses": X, "start": own[b:],
                "first_scan": np.int64(b), "session": np.int64(last), "node_base": np.int64(b * n),
                "radii": np.asarray(radii, dtype=np.float64), "iters": np.int64(iters)})
    return out


def track_lists(model, seq, sessions, located=None, radii=(2.0, 0.75), reacquire_radii=(8.0,), iters=10, min_nodes=6,
                min_matched=10, radius=0.75, tau_z=0.75):
    """The last of `sessions` consecutive near-equal sessions of `seq` (session_lists' split) tracked through the landmark
    map of the others (SG.track_in_map): the map is built on the sequence's own poses (SG.landmark_map), all of its
    landmarks take part, the odometry of the drive is the sequence's own poses.  located: the dict of localize_lists;
    when it accepted the drive's first scan the track starts from its pose, else from the stored one.
    -> dict of numpy arrays: poses, pred f64 [Q,4], matched, live, steps, flags i32 [Q], lost bool [Q], rms f64 [Q],
    node_landmark i32 [Q,N], num = (tracked, lost, longest lost run, tracks), init [1,4], from_localize, first_scan,
    session, radii, reacquire_radii, iters, min_nodes, min_matched, matched_share (the median of matched / live over the
    scans with a live node), median_trans_m / p95_trans_m against the sequence's own poses."""
    m = seq.labels.shape[0]
    bounds = np.asarray([(j * m) // int(sessions) for j in range(int(sessions))], dtype=np.int32)
    b, last = int(bounds[-1]), int(sessions) - 1
    own = metrics.planar_odometry(seq.poses)
    lm = model.landmark_map(seq.centers[:b], seq.labels[:b], own[:b], sessions=bounds[:-1], radius=radius, tau_z=tau_z)
    init = np.array(own[b:b + 1])
    given = bool(located is not None and np.asarray(located["accept"], dtype=bool).reshape(-1)[b]
                 and np.isfinite(located["pose"][b]).all())
    if given:
        init[0] = located["pose"][b]
    X, info = model.track_in_map(seq.centers[b:], seq.labels[b:], own[b:], init, lm, radii=radii, reacquire_radii=reacquire_radii,
                                 iters=iters, min_nodes=min_nodes, min_matched=min_matched, tau_z=tau_z)
    X = X.cpu().numpy()
    out = {"poses": X, "init": init, "from_localize": np.bool_(given), "first_scan": np.int64(b), "session": np.int64(last),
           "radii": np.asarray(radii, dtype=np.float64), "reacquire_radii": np.asarray(reacquire_radii, dtype=np.float64),
           "iters": np.int64(iters), "min_nodes": np.int64(min_nodes), "min_matched": np.int64(min_matched)}
    out.update({k: info[k] for k in ("pred", "matched", "live", "steps", "flags", "lost", "rms", "node_landmark", "num")})
    err = metrics.localization_errors(X, own[b:])["trans_m"]
    out["median_trans_m"], out["p95_trans_m"] = np.float64(np.median(err)), np.float64(np.percentile(err, 95))
    seen = info["live"] > 0
    out["matched_share"] = np.float64(np.median(info["matched"][seen] / info["live"][seen]) if seen.any() else 0.0)
    return out


def relocalize_lists(model, seq, sessions, radii=(2.0, 0.75), iters=10, min_nodes=6, min_inliers=12, max_base=30.0, sep=10.0,
                     ratio=0.7, radius=0.75, tau_z=0.75):
    """The scans of the last of `sessions` consecutive near-equal sessions of `seq` (session_lists' split) relocalised in
    the landmark map of the others with no prior pose (SG.relocalize_in_map): the map is built on the sequence's own
    poses (SG.landmark_map), all of its landmarks take part.
    -> dict of numpy arrays: poses f64 [Q,4] (NaN where not found), found, ambiguous bool [Q], inliers, inliers_other,
    matched, live, steps, flags i32 [Q], coarse, other f64 [Q,4], win i32 [Q,4], hypotheses i64 [Q], rms f64 [Q],
    node_landmark i32 [Q,N], num, trans_m f64 [Q] (against the sequence's own poses; NaN where not found), first_scan,
    session, radii, iters, min_nodes, min_inliers, max_base, sep, ratio, median_trans_m / max_trans_m of the found scans."""
    m = seq.labels.shape[0]
    bounds = np.asarray([(j * m) // int(sessions) for j in range(int(sessions))], dtype=np.int32)
    b, last = int(bounds[-1]), int(sessions) - 1
    own = metrics.planar_odometry(seq.poses)
    lm = model.landmark_map(seq.centers[:b], seq.labels[:b], own[:b], sessions=bounds[:-1], radius=radius, tau_z=tau_z)
    X, info = model.relocalize_in_map(seq.centers[b:], seq.labels[b:], lm, radii=radii, iters=iters, min_nodes=min_nodes,
                                      min_inliers=min_inliers, ratio=ratio, max_base=max_base, sep=sep, tau_z=tau_z)
    X = X.cpu().numpy()
    found = info["found"]
    err = np.full(X.shape[0], np.nan)
    if found.any():
        err[found] = metrics.localization_errors(X[found], own[b:][found])["trans_m"]
    out = {"poses": X, "trans_m": err, "first_scan": np.int64(b), "session": np.int64(last),
           "radii": np.asarray(radii, dtype=np.float64), "iters": np.int64(iters), "min_nodes": np.int64(min_nodes),
           "min_inliers": np.int64(min_inliers), "max_base": np.float64(max_base), "sep": np.float64(sep), "ratio": np.float64(ratio),
           "median_trans_m": np.float64(np.median(err[found]) if found.any() else np.nan),
           "max_trans_m": np.float64(err[found].max() if found.any() else np.nan)}
    out.update({k: info[k] for k in ("found", "ambiguous", "inliers", "inliers_other", "coarse", "other", "win", "hypotheses",
                                     "matched", "live", "steps", "flags", "rms", "node_landmark", "num")})
    return out


def relocalized_start(report, scans):
    """relocalize_lists' dict as the `located` argument of track_lists: the session's first scan is given its relocalised
    pose when it was found and is not ambiguous, no other scan is given one"""
    b = int(report["first_scan"])
    accept, pose = np.zeros(int(scans), dtype=bool), np.full((int(scans), 4), np.nan)
    if report["found"].size and report["found"][0] and not report["ambiguous"][0]:
        accept[b], pose[b] = True, report["poses"][0]
    return {"accept": accept, "pose": pose}


def persist_lists(model, seq, updated, max_range=50.0, margin=2.0, min_expected=5, max_seen_ratio=0.3, radius=0.75, min_count=3):
    """The drive update_lists folded in, tallied on the map it left (SG.map_persistence): `updated` is update_lists' dict -
    the records of the updated map, node_landmark and poses of the new scans, first_scan.  There is no occlusion model.
    -> dict of numpy arrays: expected, seen i32 [L], keep bool [L]; scan_expected, scan_seen, scan_live, flags i32 [Q],
    view f64 [Q]; num = (retired, landmarks judged, eligible landmarks, scans with a view); in_use_before / in_use_after
    (the landmarks with at least min_count observations, and those of them that are kept), scan_ratio_median (the median
    of scan_seen / scan_expected over the scans that expected a landmark), and the parameters."""
    b = int(updated["first_scan"])
    lm = {k: updated[k] for k in ("center", "label", "count", "first", "sessions", "spread")}
    got = model.map_persistence(seq.centers[b:], seq.labels[b:], updated["poses"], lm, node_landmark=updated["node_landmark"],
                                max_range=max_range, margin=margin, min_expected=min_expected, max_seen_ratio=max_seen_ratio,
                                radius=radius)
    out = {k: got[k].cpu().numpy() for k in ("expected", "seen", "keep")}
    out.update({k: got[k] for k in ("scan_expected", "scan_seen", "scan_live", "flags", "view")})
    in_use = np.asarray(updated["count"]) >= int(min_count)
    asked = out["scan_expected"] > 0
    out.update({"num": np.asarray(got["num"], dtype=np.int64), "in_use_before": np.int64(in_use.sum()),
                "in_use_after": np.int64((in_use & out["keep"]).sum()),
                "scan_ratio_median": np.float64(np.median(out["scan_seen"][asked] / out["scan_expected"][asked]) if asked.any() else 0.0),
                "max_range": np.float64(max_range), "margin": np.float64(margin), "min_expected": np.int64(min_expected),
                "max_seen_ratio": np.float64(max_seen_ratio), "min_count": np.int64(min_count), "first_scan": np.int64(b)})
    return out


def compact_lists(model, updated, keep=None, radius=0.75, tau_z=0.75):
    """The map update_lists left, compacted on its records alone (SG.compact_map): `updated` is update_lists' dict; keep:
    persist_lists' keep mask (None: no landmark is dropped by a mask).
    -> dict of numpy arrays: center, label, count, first, sessions, spread of the compacted map, old_to_new i32 [L] (-1 =
    dropped), node_landmark [Q,N] of update_lists' scans carried through it (landmarks.remap), num = (landmarks, dropped by
    the mask, dropped as ineligible, landmarks fused from several), landmarks_before, radius, tau_z."""
    from . import landmarks as _landmarks
    lm = {k: updated[k] for k in ("center", "label", "count", "first", "sessions", "spread")}
    got = model.compact_map(lm, keep=keep, radius=radius, tau_z=tau_z)
    out = {k: got[k].cpu().numpy() for k in ("center", "label", "count", "first", "sessions", "spread", "old_to_new")}
    out.update({"node_landmark": _landmarks.remap(np.asarray(updated["node_landmark"]), out["old_to_new"]),
                "num": np.asarray([got["num_landmarks"], got["dropped"][0], got["dropped"][1], got["fused"]], dtype=np.int64),
                "landmarks_before": np.int64(len(updated["count"])), "radius": np.float64(radius), "tau_z": np.float64(tau_z)})
    return out


def merge_lists(model, seq, sessions, radius=0.75, tau_z=0.75):
    """One landmark map per session of `seq` (session_lists' split; SG.landmark_map on the sequence's own poses), merged
    left to right on their records (SG.merge_maps: session j's bit is j, its `first` counts from its first node in the
    sequence).  The yardstick is the batch map of every session on the same poses.
    -> dict of numpy arrays: center, label, count, first, sessions, spread of the merged map, num = (landmarks, 0, dropped
    as ineligible, landmarks fused from several - all of the last merge), landmarks_per_session, fused (per merge),
    batch_landmarks, same_count (the share of the merged landmarks whose count equals that of the batch landmark holding
    their first node), radius, tau_z."""
    if int(sessions) < 2:
        raise ValueError("merge_lists: there is nothing to merge with fewer than two sessions")
    m, n = seq.labels.shape[0], seq.labels.shape[1]
    bounds = [(j * m) // int(sessions) for j in range(int(sessions))] + [m]
    own = metrics.planar_odometry(seq.poses)
    maps = [model.landmark_map(seq.centers[lo:hi], seq.labels[lo:hi], own[lo:hi], radius=radius, tau_z=tau_z)
            for lo, hi in zip(bounds[:-1], bounds[1:])]
    merged, fused, last = maps[0], [], None
    for j in range(1, int(sessions)):
        last = model.merge_maps(merged, maps[j], session_shift=j, first_base=bounds[j] * n, radius=radius, tau_z=tau_z)
        merged = last
        fused.append(last["fused"])
    batch = model.landmark_map(seq.centers, seq.labels, own, sessions=np.asarray(bounds[:-1], dtype=np.int32), radius=radius,
                               tau_z=tau_z)
    out = {name: merged[name].cpu().numpy() for name in ("center", "label", "count", "first", "sessions", "spread")}
    holder = batch["node_landmark"].cpu().numpy().reshape(-1)[out["first"]]
    same = batch["count"].cpu().numpy()[holder] == out["count"]
    out.update({"num": np.asarray([last["num_landmarks"], last["dropped"][0], last["dropped"][1], last["fused"]], dtype=np.int64),
                "landmarks_per_session": np.asarray([lm["num_landmarks"] for lm in maps], dtype=np.int64),
                "fused": np.asarray(fused, dtype=np.int64), "batch_landmarks": np.int64(batch["num_landmarks"]),
                "same_count": np.float64(same.mean() if same.size else 1.0), "radius": np.float64(radius),
                "tau_z": np.float64(tau_z)})
    return out


def consistent_lists(model, seq, values, indices, min_inliers, p_thresh, window=-1, causal=False, sessions=None,
                     max_trans=1.0, max_yaw=0.06, lever_gain=0.04, min_clique=3):
    """verify_lists' accepted closures, then the pairwise-consistent ones among them (SG.consistent_closures with the
    sequence's poses as odometry; sessions N: the frames taken as N consecutive near-equal sessions - session_lists'
    split - and closures compared only within one pair of sessions).  At most engine.CONSISTENCY_MAX_CLOSURES accepted
    closures enter the selection: beyond that the ones with the most refined inliers (ties to the earlier slot).
    -> dict of numpy arrays: rows, cols, refined of the closures that entered, consistent bool, rank, degree (one per
    closure), group_size, session_starts, accepted / consistent (counts), precision_accepted / precision_consistent
    (metrics.precision_recall_at's classes)."""
    ver = model.verify_closures(seq.centers, seq.labels, indices, values=values, min_inliers=min_inliers)
    idx = torch.as_tensor(indices).to(ver["accept"].device)
    m, k = idx.shape
    rows = torch.arange(m, device=idx.device)[:, None].expand(m, k)
    acc = ver["accept"]
    arows, acols = rows[acc], idx[acc].long()
    refined, flags, inl = ver["refined"][acc], ver["flags"][acc], ver["inliers_refined"][acc]
    if arows.numel() > _engine.CONSISTENCY_MAX_CLOSURES:
        keep = torch.argsort(-inl.long(), stable=True)[:_engine.CONSISTENCY_MAX_CLOSURES].sort().values
        arows, acols, refined, flags = arows[keep], acols[keep], refined[keep], flags[keep]
    starts = None if sessions is None else np.asarray([(j * m) // int(sessions) for j in range(int(sessions))], np.int32)
    sel = model.consistent_closures({"refined": refined, "flags": flags}, arows, acols, seq.poses, row_sessions=starts,
                                    col_sessions=starts, max_trans=max_trans, max_yaw=max_yaw, lever_gain=lever_gain,
                                    min_clique=min_clique)
    ok = sel["accept"]
    kw = dict(p_thresh=p_thresh, window=window, causal=causal)
    return {"rows": arows.cpu().numpy(), "cols": acols.cpu().numpy(), "refined": refined.cpu().numpy(),
            "consistent": ok.cpu().numpy(), "rank": sel["rank"].cpu().numpy(), "degree": sel["degree"].cpu().numpy(),
            "group_size": sel["group_size"].cpu().numpy(),
            "session_starts": np.zeros(1, np.int32) if starts is None else starts,
            "accepted": np.int64(arows.numel()), "consistent_count": np.int64(int(ok.sum())),
            "precision_accepted": np.float64(metrics.precision_recall_at(arows, acols, seq.poses, **kw)[0]),
            "precision_consistent": np.float64(metrics.precision_recall_at(arows[ok], acols[ok], seq.poses, **kw)[0])}


def hard_pairs_of(db, poses, k, p_thresh, window=-1, causal=False):
    """Every member's k hardest negatives and positives (one mining call each) -> dict of numpy arrays:
    neg_indices / neg_scores, pos_indices / pos_scores [M, k] (-1 / -inf / +inf where a frame has fewer), and per frame
    neg_above_pos: its hardest negative scores above its best positive.  The best positive is the highest of the mined
    ones: the frame's best overall when it has at most k positives (exact), else a lower bound of it."""
    from .train import NEG_DISTANCE
    ids = torch.arange(len(db))
    nv, ni = db.query_ids_hard(ids, poses, k=k, positives=False, d_pos=p_thresh, d_neg=NEG_DISTANCE, window=window,
                               causal=causal)
    pv, pi = db.query_ids_hard(ids, poses, k=k, positives=True, d_pos=p_thresh, d_neg=NEG_DISTANCE, window=window,
                               causal=causal)
    nv, ni, pv, pi = nv.cpu().numpy(), ni.cpu().numpy(), pv.cpu().numpy(), pi.cpu().numpy()
    best_pos = np.where(pi >= 0, pv, -np.inf).max(axis=1)
    has_pos, has_neg = pi[:, 0] >= 0, ni[:, 0] >= 0
    return {"neg_indices": ni, "neg_scores": nv, "pos_indices": pi, "pos_scores": pv,
            "neg_above_pos": has_pos & has_neg & (nv[:, 0] > best_pos), "exact": pi[:, -1] < 0}


if __name__ == "__main__":
    main()

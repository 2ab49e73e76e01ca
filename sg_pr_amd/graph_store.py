"""Packed graph store + whole-sequence evaluation (the caller side of the hot path).

The reference re-reads and re-pads both JSON graphs of every pair (utils.py:27-28, sg_net.py:250-299): ~0.7 ms of
host work per pair, hours for the 20 M pairs of KITTI-00.  Here every graph of a sequence is parsed ONCE into the
engine's wire format

    centers  float32 [M, node_num, 3]   zero for padded slots         (sg_net.py:262)
    labels   int32   [M, node_num]      -1   for padded slots         (sg_net.py:260)
    poses    float64 [M, 12]            the 3x4 KITTI pose rows       (utils.py:36 uses [3] and [11])

kept as one `.npz` per sequence, together with what the engine's launch plan needs (processed slots per graph ->
node_cap and the largest-first order).  `evaluate_all_pairs` then runs the sequence end to end on the GPU: embed
once per graph, dense M x M scores, F1-max from threshold counts and the loop-closure candidates - the score
matrix never leaves the device.
"""
import os
import re

import numpy as np
import torch

from . import metrics
from .sg_net import pack_graph
from .utils import read_graph


class PackedSequence:
    def __init__(self, centers, labels, poses, names):
        self.centers = np.ascontiguousarray(centers, dtype=np.float32)
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.poses = np.ascontiguousarray(poses, dtype=np.float64)
        self.names = list(names)
        m = self.labels.shape[0]
        if self.centers.shape != (m, self.labels.shape[1], 3) or self.poses.shape != (m, 12) or len(self.names) != m:
            raise ValueError("inconsistent packed sequence")

    def __len__(self):
        return self.labels.shape[0]

    @property
    def node_num(self):
        return self.labels.shape[1]

    def ragged(self, device=None):
        """The sequence as the ragged store of sgpr_embed_ragged: an `allpairs.RaggedGraphs` (centers f32 [S,3], labels
        i8 [S], host offsets i64 [M+1]) - only the real nodes, 13 bytes each instead of 16 per slot: what to keep
        resident for a whole data set and what to move across PCIe.  Accepted wherever graphs are
        (`SG.embed(rag, None)`, `AllPairsScorer.run(rag, None)`, `SequenceSet`)."""
        from .allpairs import RaggedGraphs
        return RaggedGraphs.from_padded(self.centers, self.labels, device=device)

    def save(self, path):
        np.savez_compressed(path, centers=self.centers, labels=self.labels, poses=self.poses,
                            names=np.array(self.names))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["centers"], z["labels"], z["poses"], [str(n) for n in z["names"]])


def _natural_key(name):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def pack_directory(graph_dir, node_num, number_of_labels=12, names=None):
    """Parse `<graph_dir>/*.json` (or the listed file names) once -> PackedSequence, frames in natural order."""
    if names is None:
        names = sorted((f for f in os.listdir(graph_dir) if f.endswith(".json")), key=_natural_key)
    m = len(names)
    centers = np.zeros((m, node_num, 3), dtype=np.float32)
    labels = -np.ones((m, node_num), dtype=np.int32)
    poses = np.zeros((m, 12), dtype=np.float64)
    for g, name in enumerate(names):
        d = read_graph(os.path.join(graph_dir, name))
        centers[g], labels[g] = pack_graph(d["centers"], d["nodes"], node_num, number_of_labels)
        poses[g] = np.asarray(d["pose"], dtype=np.float64).reshape(-1)[:12]
    return PackedSequence(centers, labels, poses, names)


def evaluate_all_pairs(model, seq, p_thresh=3.0, n_thresh=20.0, top_k=1, window=50, scorer=None, keep_matrix=True,
                       seq_len=1, seq_reverse="both"):
    """Whole-sequence evaluation on the device.  Returns {"f1_max", "roc_auc", "closure_scores" [M,k], "closure_frames"
    [M,k], "matrix" (device tensor: this rank's row block)}.  `scorer`: an AllPairsScorer for multi-GPU runs.
    keep_matrix=False never forms the matrix: F1-max and the area come from AllPairsScorer.pr_roc_pooled, the
    closures from Engine.score_topk (the same values), and "matrix" is None.
    seq_len > 1 (frames in trajectory order, one GPU, keep_matrix=True): the kept matrix is also sequence-matched
    (Engine.seq_filter, seq_reverse False / True / "both") and the result adds "seq_f1_max", "seq_roc_auc",
    "seq_closure_scores", "seq_closure_frames" and "seq_matrix" of the filtered scores beside the unfiltered ones
    (without the matrix: evaluate_seq_pooled)."""
    from . import allpairs
    seq_len = int(seq_len)
    if seq_len != 1 and not keep_matrix:
        raise ValueError("evaluate_all_pairs: seq_len > 1 filters the kept matrix; keep_matrix=False is not supported")
    if scorer is None:
        scorer = allpairs.AllPairsScorer(model=model)
    eng = model.engine()
    k = int(model.args.K)
    world, rank = scorer._world()
    if seq_len != 1 and world > 1:
        raise ValueError("evaluate_all_pairs: seq_len > 1 runs on one GPU (a row shard lacks its context rows)")
    lo, hi = allpairs.shard_bounds(len(seq), world, rank)
    order, cap = eng.size_order(seq.centers[lo:hi], seq.labels[lo:hi], k)
    scorer.embed_fn = lambda c, l: eng.embed(c, l, k, node_cap=cap, order=order)[0]     # noqa: E731
    pooled = scorer.pooled_all(seq.centers, seq.labels)
    if not keep_matrix:
        return _evaluate_pooled(model, seq, pooled, p_thresh, n_thresh, top_k, window, scorer)
    block = scorer.score_rows(pooled)
    err = None
    try:
        eng.check_status()                 # bad labels / broken node_cap promises are errors, not silent NaNs
    except RuntimeError as e:              # ... on EVERY rank: agreed on before the collectives of pr_roc
        err = e
    allpairs.agree_on_error(err, like=block, group=scorer.group)
    f1, auc = scorer.pr_roc(block, seq.poses, p_thresh=p_thresh, n_thresh=n_thresh)
    vals, idx = scorer.loop_closures(block, k=top_k, window=window)
    res = {"f1_max": f1, "roc_auc": auc, "closure_scores": vals, "closure_frames": idx, "matrix": block}
    if seq_len != 1:
        q = eng.seq_filter(block, seq_len, reverse=seq_reverse)
        res["seq_f1_max"], res["seq_roc_auc"] = scorer.pr_roc(q, seq.poses, p_thresh=p_thresh, n_thresh=n_thresh)
        res["seq_closure_scores"], res["seq_closure_frames"] = scorer.loop_closures(q, k=top_k, window=window)
        res["seq_matrix"] = q
    return res


def _evaluate_pooled(model, seq, pooled, p_thresh, n_thresh, top_k, window, scorer):
    from . import allpairs
    world, rank = scorer._world()
    lo, hi = allpairs.shard_bounds(len(seq), world, rank)
    err = None
    try:
        model.engine().check_status()
    except RuntimeError as e:
        err = e
    allpairs.agree_on_error(err, like=pooled, group=scorer.group)
    f1, auc = scorer.pr_roc_pooled(seq.centers, seq.labels, seq.poses, p_thresh=p_thresh, n_thresh=n_thresh,
                                   local_pooled=pooled[lo:hi], engine=model.engine())
    vals, idx = model.loop_closures(pooled[lo:hi].contiguous(), pooled, k=top_k, window=window, row0=lo)
    return {"f1_max": f1, "roc_auc": auc, "closure_scores": vals, "closure_frames": idx, "matrix": None}


def evaluate_seq_pooled(model, seq, seq_len, seq_reverse="both", p_thresh=3.0, n_thresh=20.0, top_k=1, window=50):
    """The sequence-matched half of evaluate_all_pairs(seq_len=) without the score matrix or the filtered one (one GPU;
    frames in trajectory order): {"seq_f1_max", "seq_roc_auc"} from metrics.pr_roc_seq_pooled and {"seq_closure_scores",
    "seq_closure_frames", "seq_closure_dirs"} [M,k] from Engine.score_seq_topk - the values the matrix run reports."""
    from . import allpairs, metrics
    eng = model.engine()
    k = int(model.args.K)
    order, cap = eng.size_order(seq.centers, seq.labels, k)
    pooled = eng.embed(seq.centers, seq.labels, k, node_cap=cap, order=order)[0]
    eng.check_status()
    xz = allpairs.pose_xz(seq.poses).to(pooled.device)
    f1, auc, _ = metrics.pr_roc_seq_pooled(eng, pooled, pooled, int(seq_len), pose_xz=xz, p_thresh=p_thresh,
                                           n_thresh=n_thresh, reverse=seq_reverse)
    vals, idx, dirs = eng.score_seq_topk(pooled, pooled, int(seq_len), k=top_k, window=window, reverse=seq_reverse)
    return {"seq_f1_max": f1, "seq_roc_auc": auc, "seq_closure_scores": vals, "seq_closure_frames": idx,
            "seq_closure_dirs": dirs}


def main(argv=None):
    """python -m sg_pr_amd.graph_store config.yml   - all-pairs evaluation of every `eva_batch.sequences` entry:
    packs `<graph_pairs_dir>/<seq>/` once (cached as `<output_path>/<seq>_packed.npz`), writes
    `<seq>_allpairs_F1_max.txt` and `<seq>_loop_closures.npy` (frame, best match, score).
    --no-matrix: the same outputs without ever forming the M x M score matrix (evaluate_all_pairs keep_matrix=False).
    --seq-len L [--seq-reverse off|on|both]: also the F1-max and ROC area of the sequence-matched matrix
    (`<seq>_seq_F1_max.txt`, evaluate_all_pairs seq_len=) and its closures (`<seq>_seq_loop_closures.npy`); with
    --no-matrix the same two files without the matrix or the filtered one (evaluate_seq_pooled)."""
    import sys
    from .parser_sg import sgpr_args
    from .sg_net import SGTrainer
    argv = sys.argv[1:] if argv is None else argv
    keep_matrix = "--no-matrix" not in argv
    argv = [a for a in argv if a != "--no-matrix"]
    seq_len, seq_reverse = 1, "both"
    for flag in ("--seq-len", "--seq-reverse"):
        if flag in argv:
            i = argv.index(flag)
            if i + 1 >= len(argv):
                raise SystemExit(flag + " needs a value")
            if flag == "--seq-len":
                seq_len = int(argv[i + 1])
            else:
                if argv[i + 1] not in ("off", "on", "both"):
                    raise SystemExit("--seq-reverse must be off, on or both")
                seq_reverse = {"off": False, "on": True, "both": "both"}[argv[i + 1]]
            argv = argv[:i] + argv[i + 2:]
    args = sgpr_args()
    args.load(argv[0] if argv else "./config/config.yml")
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
        if keep_matrix or seq_len == 1:
            r = evaluate_all_pairs(trainer.model, seq, p_thresh=float(args.p_thresh), keep_matrix=keep_matrix,
                                   seq_len=seq_len, seq_reverse=seq_reverse)
        else:
            r = evaluate_all_pairs(trainer.model, seq, p_thresh=float(args.p_thresh), keep_matrix=False)
            r.update(evaluate_seq_pooled(trainer.model, seq, seq_len, seq_reverse, p_thresh=float(args.p_thresh)))
        with open(os.path.join(args.output_path, sequence + "_allpairs_F1_max.txt"), "w") as f:
            f.write(str(r["f1_max"]))
        m = len(seq)
        np.save(os.path.join(args.output_path, sequence + "_loop_closures.npy"),
                np.stack((np.arange(m), r["closure_frames"][:, 0].cpu().numpy(),
                          r["closure_scores"][:, 0].cpu().numpy()), axis=1))
        print("sequence", sequence, "frames", m, "roc_auc: ", r["roc_auc"], "F1 max score", r["f1_max"])
        if seq_len != 1:
            with open(os.path.join(args.output_path, sequence + "_seq_F1_max.txt"), "w") as f:
                f.write(str(r["seq_f1_max"]))
            np.save(os.path.join(args.output_path, sequence + "_seq_loop_closures.npy"),
                    np.stack((np.arange(m), r["seq_closure_frames"][:, 0].cpu().numpy(),
                              r["seq_closure_scores"][:, 0].cpu().numpy()), axis=1))
            print("sequence", sequence, "sequence length", seq_len, "roc_auc: ", r["seq_roc_auc"], "F1 max score",
                  r["seq_f1_max"])
        results[sequence] = r["f1_max"]
    return results


if __name__ == "__main__":
    main()

"""Every call depends on its arguments alone: dirty workspaces, dirty outputs, one handle on several streams and threads,
and the binding's launch-order cache.

include/sgpr.h promises that a handle is immutable after sgpr_create, that the caller passes every workspace and that
results depend only on the arguments.  Every other GPU test runs one call at a time on workspaces from torch.empty,
which in a short process hold zeros or the leftovers of the same call: the two cases in which a kernel that reads a
counter, flag or partial list before writing it still gives the right answer.  Here the workspaces come filled with
0x00, 0xFF, 0x7F or random bytes, or are one arena that a sequence of different entry points reuses in stream order;
outputs the header says a call writes come pre-filled with 0xFF; and independent work runs on two streams and in four
threads of a fresh process.  Each result must be bit-identical (as integers, so NaN positions count) to the same call on
a zeroed workspace, and that baseline is checked against the float64 reference of tests/score_ref.py once per scoring
entry point.

Workspace and output audit: what initialises each region in the same call before any kernel reads it.

| entry point | region | initialised by |
|---|---|---|
| sgpr_embed, _capped, _ordered, _ragged, _dense, sgpr_forward_dense (tuned kernels) | redo flags, one byte per launch slot | producer: the slot's first-pass workgroup stores 0 or its request (1 / 2 / 3) for every slot it owns, the NaN path included (`request_redo`, sgpr_embed.hip) |
| | redo_count word | per-call token: stored only with a request; the second pass scans the flags only when it equals this launch's `sem_epoch` |
| | over_count word | per-call token, read by the hand-over launch (`embed_big_kernel`, auto_over 2) the same way |
| | parked first-branch rows (N > 128) | producer: written by the graph's own workgroup before it reads them back |
| | split-launch slots `sem_flag[s]` | per-call token `sem_token(sem_epoch, s)`; a consumer that does not see it hands its graph to the second pass |
| | split-launch rows `sem_tab[s]` | producer: written before `sem_flag[s]` is released |
| any-shape embed (sgpr_wide.hip + sgpr_generic.hip) | redo flags + token word ahead of the generic scratch | producer per slot + per-call token (`sem_epoch`) |
| | generic scratch (activations) | producer: each workgroup writes its graph's rows before reading them |
| sgpr_size_order | slots [G] | producer: `slots_kernel` writes one count per graph; `order_kernel` sorts in LDS |
| | d_order [G], d_info [2] (outputs) | producer: written in full by `order_kernel` |
| sgpr_score_all_pairs (tuned, bit 13) | `u_r | range partials | A'_r planes | column planes` | producer: `ntn_prep_kernel` writes every row, partial and plane the tail reads |
| sgpr_score_all_pairs (any-shape, matrix-core tail) | operands + `TailHdr` maxima | memset of the `TailHdr` (`hipMemsetAsync(hdr, 0, sizeof(TailHdr))`) before the `atomicMax` prep; operands by producer |
| sgpr_score_all_pairs_multi | per job: the all-pairs layout at a 256-byte aligned offset | producer, as for one rectangle |
| sgpr_score_pair_list | `u_r | range partials | A'_r planes | column planes` | producer: the list's prep kernel |
| sgpr_score_topk (fused) | operands | producer: `ntn_prep_kernel` |
| | partial lists `[grid][2][16][k]` values / columns | producer: a workgroup stores the lists of the row groups at both ends of its range; `topk_merge_kernel` reads only the slots of the workgroups that cover a row group |
| | d_values / d_indices (outputs) | producer: every [R][k] entry is written, (-inf, -1) where fewer than k columns qualify |
| sgpr_score_topk (wide-range, any-shape) | score block + the all-pairs workspace | producer: the block's all-pairs call; the selection reads only that block |
| every row-blocked epilogue (any-shape, matrix-core tail) | the all-pairs region's `TailHdr` | memset once per call, then a prep pass over every block; no block's scoring clears it |
| sgpr_score_above (fused) | row_ptr [R + 1] in the workspace when the caller passes none | producer: `above_scan_kernel` |
| | item flags, one byte per 16 x 256 work item | memset of `items` bytes per row block |
| | the call's range `float4` (more than one row block; also sgpr_score_positives / _threshold_counts) | memset, then `ap_range_fold_kernel` after each block's first-pass prep, before any block is scored |
| | per-row counts `cnt` | producer: pass 1 (rows inside one workgroup) or `above_fold_kernel` (rows shared between workgroups) |
| | partial counts / offsets `pcnt`, `poff` | producer: pass 1 stores the shares it owns; the fold reads only those |
| | d_count, d_row_ptr (outputs) | `above_scan_kernel` (the first block stores, later blocks add to the count the first stored); memsets when R or M is 0 |
| | d_rows / d_cols / d_values (outputs) | producer: pass 2 writes positions [0, min(count, capacity)) |
| sgpr_rows_above | counts [R], then row_ptr [R + 1] | producer: pass 1 kernel, then the scan |
| sgpr_pair_positives | d_count (output) | memset of 16 bytes; the list by atomic append after it |
| sgpr_pair_threshold_counts | one slab of counters per workgroup | producer: each workgroup stores its whole slab (no accumulation across calls) |
| | d_out [T + 3] (output) | producer: the reduction stores every word; memset when R or M is 0 |
| sgpr_f1_max | counts, control block, sizes, positive / negative histograms, second-pass sums | memset of bytes [0, `off_tpge`) |
| | `tpge` / `fpge` | producer: stored for the marked bins, and only marked bins are read |
| | marks | zeroed in LDS, copied out whole by the kernel that sets them |
| | thresholds, their info, positive list, pass-A slabs, class bytes | producer: written by the pass before the one that reads them |
| | d_result [8] (output) | memset of 64 bytes, then stores |
| sgpr_cluster_scan | node_of_root, cell hash (keys + values), instance hash, instance minima, class flags / counters | memsets (0xFF, 0xFF, 0xFF, 0x7F, 0) at the top of the call |
| | d_num_nodes, node arrays (outputs) | producer: stored by the last kernel |
| every entry point taking a handle | the status word `h->d_status` | belongs to the handle, not the call: raised by any call, reported and cleared by sgpr_check_status |

The map back end, one row per entry point; region by region, with the byte counts against the carves, in the docstring
of tests/test_gpu_map_stateless.py, which runs them under these fills.

| entry point | region | initialised by |
|---|---|---|
| sgpr_landmark_map | cell_key \\| cell_head | one memset 0xff of align256(H * 8) + align256(H * 4), the two carves; every per-node array and the per-workgroup counts by producer (`lm_transform_kernel`, `lm_flatten_kernel`) |
| sgpr_landmark_refine | acc [2][L][3] \\| scal [32] | one memset 0 of both carves; the two pose arrays by producer (`rf_fit_kernel`) |
| sgpr_landmark_align | cell_key \\| cell_head | memset 0xff of `la_table_clear_bytes(L)`, the carve of `la_table_carve`; elab and next by producer (`la_prep_landmark`) |
| sgpr_landmark_update | sums \\| q \\| sess \\| cnt \\| tally | one memset 0 of `upd_zero_bytes(L)`, the five carves; the core's part as sgpr_landmark_map; mlab, obs, centre, core_num by producer |
| sgpr_landmark_persist | elab | producer (`lp_prep_kernel`); the table regions are read only by the -DSGPR_PERSIST_SEARCH=1 build, which clears cell_key (0xff, H * 8 = its carve) and cell_cnt \\| total (0) |
| sgpr_landmark_track | cell_key \\| cell_head of each of the n_stages tables | one memset 0xff of `la_table_clear_bytes(L)` per stage; d_num by a memset 0 of 16 bytes |
| sgpr_landmark_relocalize | cell_key \\| cell_head of each of the n_stages + 2 tables | one memset 0xff of `la_table_clear_bytes(L)` per table; lab_count \\| lab_cursor and d_num by memsets 0; list, stage radii, live slots by producer |
| sgpr_landmark_merge | cell_key \\| cell_head; tally | memset 0xff of the two carves; memset 0 of 64 * 4 bytes; every per-record array by producer (`mrg_prepare_kernel`) |
| sgpr_posegraph_optimize | every region | producer: the one workgroup of `pg_solve_kernel` stores each array, counts included, before the barrier after which it is read; no memset |
"""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import score_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ["00", "ff", "7f", "random"]
BAR = 3e-6            # the bar of test_gpu_score_range.py (f16 planes and exact fp32 against float64)


# ---------------------------------------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def eng(ckpt_path):
    from sg_pr_amd import engine
    from oracle import sgpr_oracle
    e = engine.Engine(sgpr_oracle.load_checkpoint(ckpt_path), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sd(ckpt_path):
    from oracle import sgpr_oracle
    return sgpr_oracle.load_checkpoint(ckpt_path)


def _any_shape_sd():
    from sg_pr_amd import sg_net
    from sg_pr_amd.parser_sg import sgpr_args
    args = sgpr_args()
    args.filters_1, args.filters_2, args.filters_3, args.tensor_neurons, args.bottle_neck_neurons = 64, 64, 48, 16, 16
    args.node_num, args.K = 64, 10
    torch.manual_seed(5)
    sd = {k: v.detach().clone() for k, v in sg_net.SG(args, 12).eval().state_dict().items()}
    return sd, args


@pytest.fixture(scope="module")
def any_eng():
    from sg_pr_amd import engine
    sd, args = _any_shape_sd()
    e = engine.Engine(sd, dims=engine.dims_from_args(args, 12), device=0)
    assert e.any_shape
    yield e, sd
    e.close()


def _bits(x):
    """an output as integer bits on the host (NaN positions count)"""
    if isinstance(x, torch.Tensor):
        t = x.detach().contiguous().cpu()
        if t.dtype == torch.float32:
            t = t.view(torch.int32)
        elif t.dtype == torch.float64:
            t = t.view(torch.int64)
        return t.numpy().copy()
    a = np.ascontiguousarray(np.asarray(x))
    if a.dtype == np.float32:
        return a.view(np.int32).copy()
    if a.dtype == np.float64:
        return a.view(np.int64).copy()
    return a.copy()


def _flat(out):
    if isinstance(out, (tuple, list)):
        res = []
        for o in out:
            res += _flat(o)
        return res
    if out is None:
        return []
    if isinstance(out, (int, float)):
        return [np.asarray(out)]
    return [_bits(out)]


def _trim(ab):
    """score_above / rows_above with a capacity: only the first min(count, capacity) pairs are defined"""
    n = min(int(ab[3][-1]), ab[0].numel())
    return ab[0][:n], ab[1][:n], ab[2][:n], ab[3]


def _fill(nbytes, pattern, gen):
    n = max(int(nbytes), 16)
    if pattern == "random":
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    return torch.full((n,), int(pattern, 16), dtype=torch.uint8, device="cuda")


class _Poison:
    """Engine._ws replaced on ONE engine instance: every call gets a fresh buffer filled with `pattern`, or (pattern
    "arena") a view of one caller-held arena of random bytes that successive calls reuse in stream order."""

    def __init__(self, eng, pattern, seed=0, arena_bytes=0):
        self.eng, self.pattern = eng, pattern
        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(seed)
        self.arena = _fill(arena_bytes, "random", self.gen) if pattern == "arena" else None

    def _ws(self, nbytes):
        if self.arena is not None:
            assert nbytes <= self.arena.numel(), ("arena too small", nbytes)
            return self.arena[:max(int(nbytes), 16)]
        return _fill(nbytes, self.pattern, self.gen)

    def __enter__(self):
        self.eng._ws = self._ws
        return self

    def __exit__(self, *exc):
        del self.eng._ws            # back to the class's method
        return False


def _status(eng):
    from sg_pr_amd.engine import SgprError
    try:
        eng.check_status()
        return 0
    except SgprError as e:
        return e.code


def _run(eng, fn, pattern, seed=0):
    eng.check_status()
    with _Poison(eng, pattern, seed):
        out = fn()
        torch.cuda.synchronize()
    return _flat(out), _status(eng)


def _assert_same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), (what, "output", i, int((x != y).sum()) if x.shape == y.shape else
                                                              (x.shape, y.shape))


def _check_all_patterns(eng, fn, what):
    base, st0 = _run(eng, fn, "00")
    for i, p in enumerate(PATTERNS[1:]):
        got, st = _run(eng, fn, p, seed=11 + i)
        _assert_same(got, base, (what, p))
        assert st == st0, (what, p, st, st0)
    return base


# ------------------------------------------------------------------------------------------ embed entry points
def _graphs(num, n, lo, hi, seed, kitti=False, big_every=0):
    from sg_pr_amd import synth
    centers, labels, _ = synth.make_graphs(num, n, lo, hi, seed, kitti_like=kitti)
    if big_every:
        centers = centers.copy()
        centers[::big_every] *= 2000.0                     # coordinates up to 1e5: the wide-range second pass
    return centers, labels


EMBED_CASES = [
    # (id, G, node_num, nodes lo..hi, kitti-like, every n-th graph beyond the f16 range)
    ("hand-over, G > CUs", 1500, 100, 25, 90, False, 0),
    ("hand-over launch, node_num 256", 600, 256, 20, 120, False, 0),
    ("split launch, G <= 128", 96, 100, 20, 60, True, 0),
    ("split launch + redo", 24, 100, 25, 60, True, 3),
    ("G > CUs + redo", 700, 100, 25, 60, True, 5),
]


@pytest.mark.parametrize("case", EMBED_CASES, ids=[c[0] for c in EMBED_CASES])
def test_embed_entry_points_on_dirty_workspaces(eng, case):
    name, num, n, lo, hi, kitti, big = case
    centers, labels = _graphs(num, n, lo, hi, 100 + num + n, kitti, big)
    assert (num > eng.num_cus) == (num >= 600)
    eff = eng.processed_slots(centers, labels, 10)
    if hi > 64:
        assert int((eff > 64).sum()) > 0                  # the hand-over runs
    order, cap = eng.size_order(centers, labels, 10)
    rc_, rl_, ro_ = eng.to_ragged(centers, labels)
    dc, dl = torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda()
    calls = {
        "embed": lambda: eng.embed(centers, labels, 10, want_att=True, want_emb=True),
        "embed_capped": lambda: eng.embed(centers, labels, 10, node_cap=cap),
        "embed_ordered": lambda: eng.embed(centers, labels, 10, node_cap=cap, order=order),
        "embed_ordered, no promise": lambda: eng.embed(centers, labels, 10, order=order),
        "embed_ragged": lambda: eng.embed_ragged(rc_, rl_, ro_, n, 10, want_att=True),
        "embed_ragged ordered": lambda: eng.embed_ragged(rc_, rl_, ro_, n, 10, node_cap=cap, order=order),
        "size_order": lambda: eng.size_order_device(dc, dl, None, n, 10),
        "size_order ragged": lambda: eng.size_order_device(None, None, torch.from_numpy(ro_).cuda(), n, 10),
    }
    if n <= 128:
        from sg_pr_amd import synth
        feats = synth.dense_features(centers, labels)
        calls["embed_dense"] = lambda: eng.embed_dense(feats, 10, want_att=True)
        half = num // 2
        calls["forward_dense"] = lambda: eng.forward_dense(feats[:half], feats[half:2 * half], 10)
    ref = None
    for what, fn in calls.items():
        base = _check_all_patterns(eng, fn, (name, what))
        if what == "embed":
            ref = base[0]
            assert np.isfinite(ref.view(np.float32)).all(), name
        elif what.startswith("embed") and what != "embed_dense":
            assert np.array_equal(base[0], ref), (name, what, "differs from the plain embed")


def test_any_shape_embed_on_dirty_workspaces(any_eng):
    """the any-shape handle's matrix-core embed, its flags + token and the plain-fp32 kernel behind it"""
    e, _ = any_eng
    centers, labels = _graphs(300, 64, 20, 60, 41, True, 4)
    base = _check_all_patterns(e, lambda: e.embed(centers, labels, 10, want_att=True), "any-shape embed")
    assert np.isfinite(base[0].view(np.float32)).all()


# ------------------------------------------------------------------------------------------ scoring entry points
def _handles(eng, any_eng):
    """(name, engine, debug mask, pooled width, input scale)"""
    e_any, _ = any_eng
    return [("tuned", eng, 0, 32, 4.0), ("tuned, bit 13", eng, 1 << 13, 32, 4.0),
            ("any-shape", e_any, 0, 48, 1.0), ("any-shape, bit 23", e_any, 1 << 23, 48, 1.0)]


def _pooled(n, width, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, width, generator=g) * scale).cuda()


def _scoring_calls(e, rows, cols):
    r, m = rows.shape[0], cols.shape[0]
    g = np.random.default_rng(r + m)
    i1, i2 = g.integers(0, r, 2000), g.integers(0, m, 2000)
    plan = e.pair_plan(i1, i2, r, m)
    jobs = [(rows[:17], cols), (rows[:1], cols[:65]), (rows, cols[:1]), (rows[5:], cols[3:]), (rows[2:19], cols)]
    jobs = jobs + jobs[:4]                                     # more than 8: two calls of the C entry point
    return {
        "score_all_pairs": lambda: e.score_all_pairs(rows, cols),
        "score_all_pairs_multi": lambda: e.score_all_pairs_multi(jobs),
        "score_pair_list": lambda: e.score_pair_list(rows, cols, plan),
        "score_topk k=1": lambda: e.score_topk(rows, cols, k=1, window=2),
        "score_topk k=16 causal": lambda: e.score_topk(rows, cols, k=16, window=2, causal=True, row0=m - r),
        "score_above": lambda: e.score_above(rows, cols, 0.5, window=2),
    }, (i1, i2)


@pytest.mark.parametrize("hidx", range(4), ids=["tuned", "tuned, bit 13", "any-shape", "any-shape, bit 23"])
def test_scoring_entry_points_on_dirty_workspaces(eng, any_eng, sd, hidx):
    name, e, mask, width, scale = _handles(eng, any_eng)[hidx]
    e_sd = any_eng[1] if e is not eng else sd
    e.set_skip_mask(mask)
    try:
        for (r, m), mult in (((37, 131), 1.0), ((300, 1200), 1.0), ((19, 300), 1000.0)):
            rows_np = (_pooled(r, width, scale, 3 + r).cpu().numpy() * mult).astype(np.float32)
            cols_np = (_pooled(m, width, scale, 4 + m).cpu().numpy() * mult).astype(np.float32)
            rows, cols = torch.from_numpy(rows_np).cuda(), torch.from_numpy(cols_np).cuda()
            calls, (i1, i2) = _scoring_calls(e, rows, cols)
            base = {}
            for what, fn in calls.items():
                base[what] = _check_all_patterns(e, fn, (name, r, m, mult, what))
            if mult == 1.0 and r == 37:
                # the zero-workspace baseline against float64: "identical to a wrong answer" cannot pass
                ref = score_ref.tail(e_sd, rows_np, cols_np)["score"]
                mat = base["score_all_pairs"][0].view(np.float32).reshape(r, m).astype(np.float64)
                assert np.abs(mat - ref).max() <= BAR, (name, "score_all_pairs vs float64")
                pl = base["score_pair_list"][0].view(np.float32).astype(np.float64)
                assert np.abs(pl - ref[i1, i2]).max() <= BAR, (name, "score_pair_list vs float64")
                multi = [o.view(np.float32).astype(np.float64) for o in base["score_all_pairs_multi"]]
                assert np.abs(multi[0] - ref[:17]).max() <= BAR, (name, "score_all_pairs_multi vs float64")
                assert np.abs(multi[3] - ref[5:, 3:]).max() <= BAR, (name, "score_all_pairs_multi vs float64")
                v1 = base["score_topk k=1"][0].view(np.float32).reshape(r, 1)
                i1k = base["score_topk k=1"][1].reshape(r, 1)
                cc = np.arange(m)[None, :]
                ok = np.abs(cc - np.arange(r)[:, None]) > 2
                best = np.where(ok, ref, -np.inf).max(1)
                assert np.abs(v1[:, 0] - best).max() <= BAR, (name, "score_topk vs float64")
                assert (ref[np.arange(r), i1k[:, 0]] >= best - 2 * BAR).all(), (name, "score_topk index vs float64")
                n_above = int(base["score_above"][3][-1])
                want = int(((ref >= 0.5) & ok).sum())
                assert abs(n_above - want) <= int((np.abs(ref - 0.5) <= BAR).sum()), (name, "score_above count vs float64")
    finally:
        e.set_skip_mask(0)


def test_topk_rows_shared_between_workgroups(eng):
    """few rows, many columns: row groups span several workgroups, whose partial lists the merge folds"""
    rows, cols = _pooled(8, 32, 4.0, 5), _pooled(40000, 32, 4.0, 6)
    for k in (1, 16):
        for causal in (False, True):
            _check_all_patterns(eng, lambda: eng.score_topk(rows, cols, k=k, window=3, causal=causal, row0=20000),
                                ("topk shared rows", k, causal))
    # the same rows and columns through the fused score_above (shared rows: partial counts + fold)
    _check_all_patterns(eng, lambda: _trim(eng.score_above(rows, cols, 0.3, window=3, capacity=50000)), "above shared rows")


def test_above_cases_on_dirty_workspaces(eng):
    rows, cols = _pooled(700, 32, 3.0, 7), _pooled(2000, 32, 3.0, 8)
    score = eng.score_all_pairs(rows, cols)
    thr = float(torch.quantile(score[:200].reshape(-1).cpu(), 0.99))
    total = int(eng.score_above(rows, cols, thr)[3][-1])
    assert total > 1000
    for what, fn in {
        "score_above": lambda: eng.score_above(rows, cols, thr, window=20, causal=True, row0=900),
        "score_above capacity cut": lambda: _trim(eng.score_above(rows, cols, thr, capacity=total // 3)),
        "score_above count only": lambda: eng.score_above(rows, cols, thr, capacity=0),
        "rows_above": lambda: eng.rows_above(score, thr, window=20),
        "rows_above capacity cut": lambda: _trim(eng.rows_above(score, thr, capacity=total // 3)),
    }.items():
        _check_all_patterns(eng, fn, what)


def test_above_row_blocks_of_a_long_launch(eng):
    """more rows than one fused launch takes (131072): the second block continues from the first's device count"""
    base = _pooled(4541, 32, 3.0, 9)
    n = 131072 + 37
    rows = base[torch.arange(n, device="cuda") % base.shape[0]].contiguous()
    cols = base[:300].contiguous()
    thr = float(torch.quantile(eng.score_all_pairs(base[:500], cols).reshape(-1).cpu(), 0.99))
    want = eng.score_above(rows, cols, thr, window=5)
    k = int(want[3][131072]) + 3
    for causal in (False, True):
        _check_all_patterns(eng, lambda: eng.score_above(rows, cols, thr, window=5, causal=causal), ("blocks", causal))
        _check_all_patterns(eng, lambda: _trim(eng.score_above(rows, cols, thr, window=5, causal=causal, capacity=k)),
                            ("blocks, capacity", causal))


# ------------------------------------------------------------------------------------------ consumers of the matrix
@pytest.fixture(scope="module")
def seq(eng):
    from sg_pr_amd import allpairs, synth
    centers, labels, _, poses = synth.kitti_like_sequence(num_graphs=700, node_num=100, seed=9)
    order, cap = eng.size_order(centers, labels, 10)
    pooled = eng.embed(centers, labels, 10, node_cap=cap, order=order)[0]
    m = eng.score_all_pairs(pooled, pooled)
    xz = allpairs.pose_xz(poses)
    d = torch.cdist(xz.double(), xz.double())
    gt = torch.where(d <= 3, 1, torch.where(d >= 20, 0, -1)).to(torch.int8)
    return pooled, m, xz, gt


def test_metrics_on_dirty_workspaces(eng, seq):
    from sg_pr_amd import metrics
    pooled, m, xz, gt = seq
    pos_host, count_host = metrics.counts_of(m.cpu().numpy(), gt.numpy())
    u, mult = np.unique(pos_host, return_counts=True)
    above = np.concatenate((np.cumsum(mult[::-1])[::-1], [0])).astype(np.int64)
    thr = np.linspace(0.0, 1.0, 777, dtype=np.float32)
    calls = {
        "f1_max poses": lambda: eng.f1_max(m, pose_xz=xz),
        "f1_max labels, row shard": lambda: eng.f1_max(m[100:433], row0=100, pose_xz=xz),
        "pair_positives": lambda: torch.sort(eng.pair_positives(m, pose_xz=xz)[0])[0],
        "threshold counts": lambda: eng.pair_threshold_counts(m, thr, gt=gt),
        "threshold counts, ranking": lambda: eng.pair_threshold_counts(m, u[::3], pose_xz=xz, rank=(u, 3, above)),
    }
    base = {what: _check_all_patterns(eng, fn, what) for what, fn in calls.items()}
    # the zero-workspace baseline against the host computation
    np.testing.assert_array_equal(base["threshold counts"][0], count_host(thr, None)[0])
    c_host, r_host = count_host(u[::3], (u, 3, above))
    np.testing.assert_array_equal(base["threshold counts, ranking"][0], c_host)
    assert int(base["threshold counts, ranking"][2]) == r_host
    res = base["f1_max poses"][0].view(np.float64)
    keep = gt.numpy().reshape(-1) >= 0
    want = metrics.f1_max(gt.numpy().reshape(-1)[keep], m.cpu().numpy().reshape(-1)[keep])
    assert res[1] == 0 and abs(res[0] - want) <= 1e-12, (res[:2], want)


def _cluster_call(lib, pts, lab, max_nodes, ws, pre=None):
    """sgpr_cluster_scan through ctypes with a caller-made workspace; outputs pre-filled with `pre` (a byte) or zeros"""
    p = pts.shape[0]
    fill = (lambda *s, dt: torch.full(s, 0, dtype=dt, device="cuda")) if pre is None else \
        (lambda *s, dt: torch.full((int(np.prod(s)) * torch.tensor([], dtype=dt).element_size(),), pre, dtype=torch.uint8,
                                   device="cuda").view(dt).view(*s))
    centers, nlab, nsize = fill(max_nodes, 3, dt=torch.float64), fill(max_nodes, dt=torch.int32), fill(max_nodes, dt=torch.int32)
    pnode, count = fill(p, dt=torch.int32), fill(1, dt=torch.int32)
    rc = lib.sgpr_cluster_scan(_dptr(pts), pts.shape[1], _dptr(lab), p, max_nodes, _dptr(centers), _dptr(nlab), _dptr(nsize),
                               _dptr(pnode), _dptr(count), _dptr(ws), ws.numel(),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.sgpr_last_error()
    torch.cuda.synchronize()
    n = int(count.item())
    return n, centers[:n], nlab[:n], nsize[:n], pnode


def test_cluster_scan_on_dirty_workspaces_and_outputs():
    from sg_pr_amd import engine, synth
    lib = engine.load_library()
    pts_np, lab_np = synth.labelled_scan(seed=3, scale=0.5)
    pts = torch.from_numpy(pts_np).cuda()
    lab = torch.from_numpy(lab_np.view(np.int32)).cuda()
    want = engine.cluster_scan(pts, lab, want_point_node=True)
    n_want = want[0].shape[0]
    assert n_want > 5
    nbytes = int(lib.sgpr_cluster_workspace_bytes(pts.shape[0]))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    for pattern in PATTERNS:
        for pre in (None, 0xFF):
            got = _cluster_call(lib, pts, lab, 1024, _fill(nbytes, pattern, gen), pre)
            assert got[0] == n_want, (pattern, pre)
            for g_, w_ in zip(got[1:], want):
                assert np.array_equal(_bits(g_), _bits(w_)), (pattern, pre)


# ------------------------------------------------------------------------------------------ leftover arena
def test_one_arena_reused_by_a_sequence_of_entry_points(eng, seq):
    """a C caller with one scratch buffer: embed -> score_all_pairs -> score_topk -> score_above -> f1_max ->
    score_pair_list -> embed, all on one arena, stream-ordered; every result equals its zero-workspace baseline"""
    pooled_seq, m_seq, xz, gt = seq
    centers, labels = _graphs(1500, 100, 25, 90, 3, False, 7)
    rows, cols = _pooled(300, 32, 4.0, 1), _pooled(1200, 32, 4.0, 2)
    g = np.random.default_rng(5)
    plan = eng.pair_plan(g.integers(0, 300, 3000), g.integers(0, 1200, 3000), 300, 1200)
    seq_calls = [
        ("embed", lambda: eng.embed(centers, labels, 10, want_att=True)),
        ("score_all_pairs", lambda: eng.score_all_pairs(rows, cols)),
        ("score_topk", lambda: eng.score_topk(rows, cols, k=16, window=2, causal=True, row0=900)),
        ("score_above", lambda: _trim(eng.score_above(rows, cols, 0.5, window=2, capacity=100000))),
        ("f1_max", lambda: eng.f1_max(m_seq, pose_xz=xz)),
        ("score_pair_list", lambda: eng.score_pair_list(rows, cols, plan)),
        ("embed again", lambda: eng.embed(centers[:96], labels[:96], 10)),
    ]
    base = [_run(eng, fn, "00") for _, fn in seq_calls]
    for seed in (1, 2):
        eng.check_status()
        with _Poison(eng, "arena", seed, arena_bytes=64 << 20):
            outs = [_flat(fn()) for _, fn in seq_calls]
            torch.cuda.synchronize()
        st = _status(eng)
        for (what, _), got, (want, st0) in zip(seq_calls, outs, base):
            _assert_same(got, want, ("arena", seed, what))
        assert st == 0 and all(s0 == 0 for _, s0 in base), (st, [s0 for _, s0 in base])


# ------------------------------------------------------------------------------------------ dirty outputs (C-ABI)
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dptr(t):
    """a DEVICE pointer for a direct C-ABI call (a host tensor here would hand the kernel a host address)"""
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous(), "device tensor expected"
    return ctypes.c_void_p(t.data_ptr())


def _ff(n, dtype):
    size = torch.tensor([], dtype=dtype).element_size()
    return torch.full((max(int(n), 1) * size,), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)


def test_outputs_prefilled_with_ff(eng, seq):
    lib = eng.lib
    h = eng._h
    pooled_seq, m_seq, xz, gt = seq
    xz_d = xz.cuda()                 # (the poses live on the host; the engine methods upload them)
    rows, cols = _pooled(300, 32, 4.0, 11), _pooled(1200, 32, 4.0, 12)
    r, m = 300, 1200
    # score_topk: causal from row0 0, so the first rows have fewer than k columns (short rows)
    for k in (1, 16):
        wv, wi = eng.score_topk(rows, cols, k=k, window=2, causal=True)
        assert bool((wi[:3] == -1).any())
        v, ix = _ff(r * k, torch.float32), _ff(r * k, torch.int32)
        nb = eng.score_topk_workspace_bytes(r, m, k, True)
        ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
        rc = lib.sgpr_score_topk(h, _dptr(rows), r, _dptr(cols), m, None, 0, 2, 1, k, _dptr(v), _dptr(ix), _dptr(ws), nb, _stream())
        assert rc == 0
        assert np.array_equal(_bits(v.view(r, k)), _bits(wv)) and torch.equal(ix.view(r, k), wi), ("topk", k)
    # score_above: pairs up to the count, the row pointer and the count; and without a row pointer
    thr = 0.5
    wr, wc, wv, wrp = eng.score_above(rows, cols, thr, window=2)
    n = wr.numel()
    assert n > 100
    nb = eng.score_above_workspace_bytes(r, m)
    ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
    for with_rp in (True, False):
        o_r, o_c, o_v = _ff(n + 64, torch.int32), _ff(n + 64, torch.int32), _ff(n + 64, torch.float32)
        rp, cnt = _ff(r + 1, torch.int64), _ff(1, torch.int64)
        rc = lib.sgpr_score_above(h, _dptr(rows), r, _dptr(cols), m, None, 0, 2, 0, thr, _dptr(o_r), _dptr(o_c), _dptr(o_v),
                                  n + 64, _dptr(rp) if with_rp else None, _dptr(cnt), _dptr(ws), nb, _stream())
        assert rc == 0
        assert int(cnt.item()) == n
        assert torch.equal(o_r[:n], wr) and torch.equal(o_c[:n], wc) and np.array_equal(_bits(o_v[:n]), _bits(wv))
        if with_rp:
            assert torch.equal(rp, wrp)
    # the same on a resident matrix (sgpr_rows_above)
    score = eng.score_all_pairs(rows, cols)
    nb = eng.rows_above_workspace_bytes(r, m)
    ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
    o_r, o_c, o_v = _ff(n, torch.int32), _ff(n, torch.int32), _ff(n, torch.float32)
    rp, cnt = _ff(r + 1, torch.int64), _ff(1, torch.int64)
    rc = lib.sgpr_rows_above(h, _dptr(score), r, m, m, None, 0, 2, 0, thr, _dptr(o_r), _dptr(o_c), _dptr(o_v), n, _dptr(rp),
                             _dptr(cnt), _dptr(ws), nb, _stream())
    assert rc == 0
    assert int(cnt.item()) == n and torch.equal(rp, wrp) and torch.equal(o_r, wr) and torch.equal(o_c, wc)
    # f1_max result
    want = eng.f1_max(m_seq, pose_xz=xz)
    res = _ff(8, torch.float64)
    nb = int(lib.sgpr_f1_max_workspace_bytes(h, 700, 700))
    ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
    rc = lib.sgpr_f1_max(h, _dptr(m_seq), 700, 700, 700, 0, _dptr(xz_d), 3.0, 20.0, None, 700, _dptr(res), _dptr(ws), nb, _stream())
    assert rc == 0 and np.array_equal(_bits(res), _bits(want))
    # the threshold counts (+ the ranking sum)
    thr_np = np.linspace(0.0, 1.0, 777, dtype=np.float32)
    want_c, want_bad, _ = eng.pair_threshold_counts(m_seq, thr_np, gt=gt)
    t = thr_np.size
    out = _ff(t + 3, torch.int64)
    thr_d = torch.from_numpy(thr_np).cuda()
    gt_d = gt.cuda()
    nb = int(lib.sgpr_pair_threshold_counts_workspace_bytes(h, t))
    ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
    rc = lib.sgpr_pair_threshold_counts(h, _dptr(m_seq), 700, 700, 700, 0, None, 3.0, 20.0, _dptr(gt_d), 700, _dptr(thr_d), t,
                                        None, 0, None, _dptr(out), _dptr(ws), nb, _stream())
    assert rc == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:t + 1], want_c) and int(got[t + 1]) == want_bad
    # pair_positives: the count
    want_pos, want_bad = eng.pair_positives(m_seq, pose_xz=xz)
    cnt = _ff(2, torch.int64)
    plist = _ff(want_pos.numel() + 16, torch.float32)
    rc = lib.sgpr_pair_positives(h, _dptr(m_seq), 700, 700, 700, 0, _dptr(xz_d), 3.0, 20.0, None, 700, _dptr(plist),
                                 plist.numel(), _dptr(cnt), _stream())
    assert rc == 0
    assert cnt.tolist() == [want_pos.numel(), want_bad]
    assert torch.equal(torch.sort(plist[:want_pos.numel()])[0], torch.sort(want_pos)[0])
    # size_order's order and info
    centers, labels = _graphs(900, 100, 25, 90, 13)
    dc, dl = torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda()
    w_order, w_info = eng.size_order_device(dc, dl, None, 100, 10)
    order, info = _ff(900, torch.int32), _ff(2, torch.int32)
    nb = int(lib.sgpr_size_order_workspace_bytes(900))
    ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
    rc = lib.sgpr_size_order(h, _dptr(dc), _dptr(dl), None, 900, 100, 10, _dptr(order), _dptr(info), _dptr(ws), nb, _stream())
    assert rc == 0 and torch.equal(order, w_order) and torch.equal(info, w_info)
    eng.check_status()


# ------------------------------------------------------------------------------------------ two streams, one thread
def test_two_streams_one_engine(eng, seq):
    pooled_seq, m_seq, xz, gt = seq
    ca, la = _graphs(1500, 100, 25, 90, 21, False, 9)
    cb, lb = _graphs(900, 100, 20, 70, 22, True)
    rcb, rlb, rob = eng.to_ragged(cb, lb)
    dca, dla = torch.from_numpy(ca).cuda(), torch.from_numpy(la).cuda()
    rcb, rlb, rob = (torch.from_numpy(x).cuda() for x in (rcb, rlb, rob))
    rows_a, cols_a = _pooled(300, 32, 4.0, 31), _pooled(1200, 32, 4.0, 32)
    rows_b, cols_b = _pooled(250, 32, 4.0, 33), _pooled(1700, 32, 4.0, 34)
    m_b = m_seq.clone()
    torch.cuda.synchronize()

    def work_a():
        p = eng.embed(dca, dla, 10, auto_order=False)[0]
        s = eng.score_all_pairs(rows_a, cols_a)
        v, i = eng.score_topk(rows_a, cols_a, k=8, window=2)
        return [p, s, v, i]

    def work_b():
        p = eng.embed_ragged(rcb, rlb, rob, 100, 10)[0]
        ab = _trim(eng.score_above(rows_b, cols_b, 0.5, capacity=200000))
        f = eng.f1_max(m_b, pose_xz=xz)            # (synchronises stream B alone: its result is read on the host)
        return [p, *ab, f]

    serial = _flat(work_a()) + _flat(work_b())
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        with torch.cuda.stream(sa):
            out_a = work_a()
        with torch.cuda.stream(sb):
            out_b = work_b()
        with torch.cuda.stream(sa):
            out_a2 = work_a()
        torch.cuda.synchronize()
        _assert_same(_flat(out_a) + _flat(out_b), serial, "two streams")
        _assert_same(_flat(out_a2), serial[:len(_flat(out_a2))], "two streams, again")
    eng.check_status()


# ------------------------------------------------------------------------------------------ threads, fresh process
_THREAD_CHILD = textwrap.dedent(r"""
    import ctypes, sys, threading
    import numpy as np, torch
    sys.path.insert(0, sys.argv[1])
    from sg_pr_amd import engine
    from oracle import sgpr_oracle
    data = dict(np.load(sys.argv[3]))
    eng = engine.Engine(sgpr_oracle.load_checkpoint(sys.argv[2]), device=0)
    nthreads = int(data["nthreads"])

    def bits(t):
        t = t.detach().contiguous().cpu()
        return (t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t).numpy()

    def sequence(i, s):
        c = torch.from_numpy(data["c%d" % i]).cuda()
        l = torch.from_numpy(data["l%d" % i]).cuda()
        rows = torch.from_numpy(data["rows%d" % i]).cuda()
        cols = torch.from_numpy(data["cols%d" % i]).cuda()
        p = eng.embed(c, l, 10)[0]
        pp = eng.embed(data["c%d" % i], data["l%d" % i], 10)[0]
        sc = eng.score_all_pairs(rows, cols)
        v, ix = eng.score_topk(rows, cols, k=4, window=2)
        ab = eng.score_above(rows, cols, 0.5, capacity=100000)
        n = min(int(ab[3][-1]), 100000)
        ab = (ab[0][:n], ab[1][:n], ab[2][:n], ab[3])
        f1 = eng.f1_max(sc, gt=torch.from_numpy(data["gt%d" % i]).cuda())
        return [p, pp, sc, v, ix, *ab, torch.from_numpy(f1)]

    errors = []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for rep in range(3):
                    out = sequence(i, s)
                    s.synchronize()
                    for j, o in enumerate(out):
                        assert np.array_equal(bits(o), data["want%d_%d" % (i, j)]), ("thread", i, "rep", rep, "output", j)
                    # a host-refused call: the message read back is this thread's own (sgpr_last_error is thread-local)
                    r = 40 + 17 * i
                    rows = torch.zeros(r, 32, device="cuda")
                    need = int(eng.lib.sgpr_score_all_pairs_workspace_bytes(eng._h, r, 64))
                    small = torch.zeros(16, dtype=torch.uint8, device="cuda")
                    rc = eng.lib.sgpr_score_all_pairs(eng._h, engine._ptr(rows), r, engine._ptr(rows), 64, engine._ptr(rows),
                                                      64, engine._ptr(small), 16, ctypes.c_void_p(s.cuda_stream))
                    msg = eng.lib.sgpr_last_error().decode()
                    assert rc == -7 and ("workspace of %d bytes" % need) in msg, (i, rc, msg, need)
                    if i == 0:
                        try:
                            eng.embed(data["c0"][:3], data["l0"][:3], 200)
                            raise AssertionError("k > N was accepted")
                        except engine.SgprError as e:
                            assert e.code == -4, str(e)
        except BaseException as e:
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(nthreads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    eng.check_status()
    assert not errors, errors
    print("threads ok")
""")


@pytest.mark.timeout(600)
def test_threads_in_a_fresh_process(eng, tmp_path, ckpt_path):
    """4 threads on one Engine, each on its own stream with its own data, a fixed sequence 3 times, in a process whose
    first launch of every kernel (and its LDS-limit once-flag) happens concurrently; one thread also makes host-refused
    calls.  Results must be the bits the serial run here computes."""
    from sg_pr_amd import synth
    data = {"nthreads": np.int32(4)}
    for i, (num, lo, hi) in enumerate(((300, 25, 90), (96, 20, 60), (600, 25, 60), (40, 30, 100))):
        c, l, _ = synth.make_graphs(num, 100, lo, hi, 500 + i, kitti_like=(i % 2 == 1))
        data["c%d" % i], data["l%d" % i] = c, l
        rows, cols = _pooled(100 + 50 * i, 32, 4.0, 600 + i), _pooled(500 + 100 * i, 32, 4.0, 700 + i)
        data["rows%d" % i], data["cols%d" % i] = rows.cpu().numpy(), cols.cpu().numpy()
        g = np.random.default_rng(i)
        data["gt%d" % i] = g.choice(np.array([-1, 0, 1], dtype=np.int8), size=(rows.shape[0], cols.shape[0]), p=[0.1, 0.8, 0.1])
        dc, dl = torch.from_numpy(c).cuda(), torch.from_numpy(l).cuda()
        p = eng.embed(dc, dl, 10)[0]
        pp = eng.embed(c, l, 10)[0]
        sc = eng.score_all_pairs(rows, cols)
        v, ix = eng.score_topk(rows, cols, k=4, window=2)
        ab = _trim(eng.score_above(rows, cols, 0.5, capacity=100000))
        f1 = eng.f1_max(sc, gt=torch.from_numpy(data["gt%d" % i]).cuda())
        for j, o in enumerate([p, pp, sc, v, ix, *ab, torch.from_numpy(f1)]):
            data["want%d_%d" % (i, j)] = _bits(o)
    eng.check_status()
    path = str(tmp_path / "threads.npz")
    np.savez(path, **data)
    proc = subprocess.run([sys.executable, "-c", _THREAD_CHILD, REPO, ckpt_path, path], capture_output=True, text=True,
                          timeout=500)
    assert proc.returncode == 0 and "threads ok" in proc.stdout, (proc.returncode, proc.stdout[-3000:], proc.stderr[-3000:])


# ------------------------------------------------------------------------------------------ the binding's order cache
def _resident_batch(seed=61, num=1200, lo=20, hi=50):
    centers, labels = _graphs(num, 100, lo, hi, seed, True)
    return centers, labels


def test_order_cache_under_inference_mode(eng):
    centers, labels = _resident_batch()
    assert centers.shape[0] > eng.num_cus
    with torch.inference_mode():
        dc, dl = torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda()
        assert dc.is_inference()
        want = eng.embed(dc, dl, 10, auto_order=False)[0]
        first = eng.embed(dc, dl, 10)[0]
        torch.cuda.synchronize()
        second = eng.embed(dc, dl, 10)[0]                       # a hit
        assert torch.equal(first, want) and torch.equal(second, want)
        # an in-place change of inference tensors: the (stale) order is still a permutation - same bits as the plain call
        dl[7, 60:] = 3
        dc[7, 60:] = 1.5
        changed = eng.embed(dc, dl, 10)[0]
        assert torch.equal(changed, eng.embed(dc, dl, 10, auto_order=False)[0])
    eng.check_status()


@pytest.mark.parametrize("how", ["data.copy_", "dlpack"])
def test_order_cache_after_a_write_torch_does_not_track(eng, how):
    """A graph grows past the cached node_cap through a write that leaves the version counters as they were: the default
    call must not promise the old cap (before: NaN rows and SGPR_E_NODES)."""
    centers, labels = _resident_batch(62)
    dc, dl = torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda()
    eng.embed(dc, dl, 10)
    torch.cuda.synchronize()
    cap = eng._cached_order(dc, dl, 10)[1]
    assert 0 < cap <= 64                                        # the cache knows a cap below node_num
    eng.embed(dc, dl, 10)
    v = (dc._version, dl._version)
    grown_c, grown_l = centers.copy(), labels.copy()
    big_c, big_l = _graphs(4, 100, 95, 100, 63)
    grown_c[10:14], grown_l[10:14] = big_c, big_l               # four graphs of 95..100 nodes
    gc, gl = torch.from_numpy(grown_c).cuda(), torch.from_numpy(grown_l).cuda()
    if how == "data.copy_":
        dc.data.copy_(gc)
        dl.data.copy_(gl)
    else:
        torch.utils.dlpack.from_dlpack(torch.utils.dlpack.to_dlpack(dc)).copy_(gc)
        torch.utils.dlpack.from_dlpack(torch.utils.dlpack.to_dlpack(dl)).copy_(gl)
    assert (dc._version, dl._version) == v                      # torch did not see the write
    got = eng.embed(dc, dl, 10)[0]
    want = eng.embed(dc, dl, 10, auto_order=False)[0]
    assert torch.isfinite(got).all(), "NaN rows: the stale node_cap was promised"
    assert torch.equal(got, want)
    eng.check_status()


def test_order_cache_hit_on_another_stream_waits(eng, monkeypatch):
    centers, labels = _resident_batch(64)
    dc, dl = torch.from_numpy(centers).cuda(), torch.from_numpy(labels).cuda()
    want = eng.embed(dc, dl, 10, auto_order=False)[0]
    torch.cuda.synchronize()
    waits = []
    real = torch.cuda.Stream.wait_event

    def spy(self, event):
        waits.append((self.cuda_stream, event))
        return real(self, event)

    monkeypatch.setattr(torch.cuda.Stream, "wait_event", spy)
    a = eng.embed(dc, dl, 10)[0]                                # the order is made on the current stream (a miss)
    assert not waits
    sb = torch.cuda.Stream()
    with torch.cuda.stream(sb):
        b = eng.embed(dc, dl, 10)[0]                            # a hit from stream B: waits for the order's event
    assert len(waits) == 1 and waits[0][0] == sb.cuda_stream
    again = eng.embed(dc, dl, 10)[0]                            # a hit on the stream that made it: no wait
    assert len(waits) == 1
    torch.cuda.synchronize()
    assert torch.equal(a, want) and torch.equal(b, want) and torch.equal(again, want)
    eng.check_status()

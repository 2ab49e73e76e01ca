"""The map back end depends on its arguments alone: the nine workspace-taking entry points on
workspaces filled with 0x00, 0xFF, 0x7F and random bytes, with outputs pre-filled with 0xFF and with 0x5A, on the
leftovers of a larger map, on one arena that the pipeline's chain of calls reuses, and two at a time on two streams.
Every comparison is to the bit against the NumPy references (tests/landmark*_ref.py, tests/posegraph_ref.py), NaN as
bytes, the margin behind every output untouched; nothing is compared with another run of the library.

Why 0xFF alone (the fill of every older map test) is not enough.  The cell tables are cleared to 0xFF by the calls
themselves (an empty key, the end of a list), so a 0xFF workspace already is what a clear leaves: a clear that is missing,
short or misplaced shows only under another fill, and there `table_insert` / `table_find` may never reach an empty slot -
which is why the audit below was made by reading before the first run.  The counters cleared to 0 show under 0xFF and not
under 0x00.  And an int32 of 0xFFFFFFFF is -1, the value of a dead slot of d_node_landmark and of d_win without a
hypothesis: under a 0xFF prefill a kernel that skipped those stores would pass.  0x5A5A5A5A (1515870810, or 3.1e+127 as a
double) is no result of any of these calls.

Workspace audit, from the host functions: every carved region, and what initialises it in the same call before a kernel
reads it.  H = table_slots(n) >= 1024 is a power of two, so H * 8 and H * 4 are multiples of 256 and align256 changes
neither.  No region without an initialiser was found, and no clear shorter than its carve.

| entry point | region (carve) | initialised by |
|---|---|---|
| sgpr_landmark_map (lm_core_launch, P = G N) | m, sum [P][3]; lab, parent, cnt, id, q, sess [P] | producer: `lm_transform_kernel` stores every slot p < P, dead nodes included |
| | next [P] | producer: `lm_transform_kernel` (-1 of a dead node, the old list head of a live one); `lm_flatten_kernel` rewrites it for live nodes |
| | cell_key [H] \\| cell_head [H] | one memset 0xff of align256(H * 8) + align256(H * 4) bytes = the two carves |
| | blk_roots, blk_live [B] | producer: thread 0 of every workgroup of `lm_flatten_kernel` |
| | d_node_landmark, d_num (outputs) | producer: -1 by `lm_transform_kernel` for dead nodes, the id by `lm_spread_kernel` for live ones; `lm_scan_kernel` |
| sgpr_landmark_refine | acc [2][L][3] \\| scal [32] | one memset 0 of rf_acc_bytes(L) + align256(32 * 8) = the two carves; `rf_fit_kernel` re-clears the idle set, `rf_accumulate_kernel` the (Q, n) pair it has read |
| | Xw[0], Xw[1] [G][4] | producer: `rf_fit_kernel` of step k writes Xw[(k + 1) & 1] for every scan before step k + 1 reads it |
| sgpr_landmark_align | elab [L] | producer: `la_prep_landmark` for every i < L |
| | next [L] | producer: `la_prep_landmark` for eligible landmarks; only those are on a list |
| | cell_key \\| cell_head | memset 0xff of la_table_clear_bytes(L) = align256(H * 8) + align256(H * 4), the carve of la_table_carve |
| | d_node_landmark (output) | producer: `la_fit_scan` stores every slot of the row at every step (-1 dead, -2 unmatched), the whole row -1 for a non-finite pose |
| sgpr_landmark_update | the core's part (first lm_core_workspace_bytes(P) bytes) | as sgpr_landmark_map |
| | mlab, obs [P] | producer: `upd_classify_kernel` for every p < P |
| | sum [L][3] \\| q \\| sess [L] \\| cnt [L] \\| tally [64] | one memset 0 of upd_zero_bytes(L) = the five carves in order |
| | centre [L][3] | producer: `upd_centre_kernel` for every landmark with n1 > 0; read only for those |
| | core_num [64] | producer: the core's `lm_scan_kernel` (its d_num) |
| | d_node_landmark (output) | producer: the core (-1 for every node that is not new, the id of a new one), then `upd_merge_kernel` for observations |
| sgpr_landmark_persist (the build: SGPR_PERSIST_SEARCH == 2) | elab [L] | producer: `lp_prep_kernel` for every i < L |
| | lslot, item [L]; cell_key, cell_pos, cell_cnt [H]; total | not read in this build.  In the table build: memset 0xff of H * 8 (= align256(H * 8), see above) on cell_key, memset 0 of align256(H * 4) + 256 on cell_cnt \\| total; cell_pos by `lp_offsets_kernel` for used cells, lslot and item by `lp_prep_kernel` / `lp_fill_kernel` for eligible landmarks |
| | d_expected, d_seen, d_num (outputs) | producer: zeroed by `lp_prep_kernel` before the tallies add to them |
| sgpr_landmark_track | n_stages x (elab, next, cell_key \\| cell_head) | per stage: as sgpr_landmark_align, one memset 0xff of la_table_clear_bytes(L) on that stage's cell_key; `lt_prep_kernel` has one grid row per stage |
| | d_num (output) | memset 0 of 16 bytes, then integer atomics |
| | d_node_landmark (output) | producer: `la_fit_scan` of the last stage run; the whole row -1 for a track whose start is not finite |
| sgpr_landmark_relocalize | t_in, pair, t[0 .. n_stages): n_stages + 2 tables | one memset 0xff of la_table_clear_bytes(L) on the cell_key of EACH table; elab by `lr_prep_kernel` (one launch per table; the pair table's elab slice is `list`), next by the prep for eligible landmarks |
| | list [L] (= pair.elab) | producer: `lr_list_kernel` fills [0, eligible landmarks); only those are read |
| | lab_count \\| lab_cursor [2][64] | memset 0 of 2 * 64 * 4 bytes; the carve's padding is not read |
| | stage_radius [n_stages][64] | producer: `lr_prep_kernel` of launch 1 + k stores the n_labels radii of stage k; a label >= n_labels is never looked up |
| | live [Q N] (N > 256 only) | producer: the scan's workgroup compacts its live slots before it reads them |
| | d_num (output) | memset 0 of 16 bytes, then integer atomics |
| | d_node_landmark, d_win (outputs) | producer: `la_fit_scan` when found, else -2 / -1 per slot; d_win = -1 four times without a hypothesis |
| sgpr_landmark_merge (T = L_a + L_b) | p, sum [T][3]; cnt, q, sess, lab, parent, next, members, first, id [T] | producer: `mrg_prepare_kernel` stores every slot t < T |
| | centre [T][3] | producer: `mrg_record_kernel` for roots of several members; read only for those |
| | cell_key \\| cell_head | one memset 0xff of align256(H * 8) + align256(H * 4) = the two carves |
| | blk_roots [B] | producer: thread 0 of every workgroup of `mrg_flatten_kernel` |
| | tally [64] | memset 0 of 64 * 4 bytes = the carve |
| sgpr_posegraph_optimize | g, t, ozr, ozt, pos, slot, cntH, cntT [M] | producer: the first loop of `pg_solve_kernel`, every k < M (cntH / cntT zeroed there, counted by atomics after a barrier) |
| | offH, offT [M + 1]; free [M] | producer: the exclusive scans, every k <= M |
| | live [C]; czr, czt, cwr, cwt [C] | producer: the closure loop, `live` for every p < C, the rest for live closures; only live closures are listed |
| | listH, listT [C] | producer: filled from the counts, then sorted |
| | r, p, Ap, zv, diag [M] | producer: `pg_stage` writes each before the first dot product or operator that reads it |
| | Y, L, PIV, CPL [64][n_seg] | producer: `pg_stage` stores Y at slot[k] of every scan and L, PIV, CPL at every position j < len of every segment; `pg_precondition` reads those only |

Outputs that a prefill could fake.  0xFF: every int32 field that can be -1 - d_node_landmark of map, align, update, track,
relocalise; d_win; d_old_to_new of merge.  sgpr_landmark_refine, sgpr_landmark_persist and sgpr_posegraph_optimize have no
output field that can equal either prefill (poses, costs and residuals are no 0xFF.. NaN of that payload or 3.1e+127;
counts and flags are small and non-negative; d_keep is 0 or 1), so for them the prefills only guard the margins and the
Q N == 0 rule.  test_reference_holds_the_values_a_prefill_could_fake asserts on the CPU that the chosen cases hold those
values."""
import functools
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_align_ref as aref  # noqa: E402
import landmark_merge_ref as mref  # noqa: E402
import landmark_persist_ref as pref  # noqa: E402
import landmark_ref as lref  # noqa: E402
import landmark_refine_ref as rref  # noqa: E402
import landmark_relocalize_ref as rlref  # noqa: E402
import landmark_track_ref as tref  # noqa: E402
import landmark_update_ref as uref  # noqa: E402
import posegraph_ref as pgref  # noqa: E402
import test_gpu_landmark_align as t_align  # noqa: E402
import test_gpu_landmark_merge as t_merge  # noqa: E402
import test_gpu_landmark_persist as t_persist  # noqa: E402
import test_gpu_landmark_refine as t_refine  # noqa: E402
import test_gpu_landmark_relocalize as t_reloc  # noqa: E402
import test_gpu_landmark_track as t_track  # noqa: E402
import test_gpu_landmark_update as t_update  # noqa: E402
import test_gpu_landmarks as t_map  # noqa: E402
import test_gpu_posegraph as t_pg  # noqa: E402

gpu = pytest.mark.gpu

F32 = np.float32
QNAN = aref.QNAN
ENTRIES = ("map", "refine", "align", "update", "persist", "track", "relocalize", "merge", "posegraph")
# the entry points that carve a cell table.  persist carves one but the build does not read it (SGPR_PERSIST_SEARCH == 2):
# its runs here exercise elab and the outputs only, and the two clears of its table build are covered by reading alone
TABLED = ("map", "align", "update", "persist", "track", "relocalize", "merge")
SIZES = ("small", "large")
WS_FILLS = (0x00, 0xFF, 0x7F, "random")
OUT_FILLS = (0xFF, 0x5A)
# (scans, slots, landmarks): a table of 1024 slots (L, T, G N <= 512) and a larger one
SHAPE = {"small": (5, 100, 500), "large": (7, 130, 1100)}
RECORD = uref.RECORD


# ------------------------------------------------------------------ the cases: (arguments, keywords) of the reference
@functools.lru_cache(maxsize=None)
def scans(size):
    """update_ref.make_case at the size: scans that observe a made-up map from perturbed poses, their association"""
    Q, N, L = SHAPE[size]
    return uref.make_case(Q, N, L, seed=41 if size == "small" else 43)


@functools.lru_cache(maxsize=None)
def case(entry, size):
    Q, N, L = SHAPE[size]
    seed = 7 if size == "small" else 11
    if entry == "merge":
        return (mref.random_case(300, 200, seed) if size == "small" else mref.random_case(700, 400, seed),), {}
    if entry == "refine":
        *args, use = t_refine.make_case(Q, N, seed)
        fixed = np.zeros(Q, np.uint8)
        fixed[0] = 1
        return tuple(args) + (use,), dict(fixed=fixed, iters=3)
    if entry == "posegraph":
        X, starts, rows, cols, T = t_pg.loop_map(seed, (40, 30) if size == "small" else (300, 0, 250), 20 if size == "small" else 80)
        return (X, rows, cols, T), dict(starts=starts, max_iters=40)
    if entry == "persist":
        return tuple(pref.make_case(Q, N, L, seed)), dict(min_expected=2)
    centers, lab, poses, assoc, lm = scans(size)
    use = (np.random.default_rng(seed).random(L) < 0.9).astype(np.uint8)
    if entry == "map":
        return (centers, lab, poses), dict(starts=np.array([0, 2], np.int32))
    if entry == "align":
        bad = poses.copy()
        bad[1, 2] = np.nan                                           # a scan whose pose is not finite: its whole row is -1
        return (centers, lab, bad, lm["center"], lm["label"]), dict(lm_use=use, iters=3)
    if entry == "update":
        return (centers, lab, poses, assoc, lm), dict(session_base=2, starts=np.array([0, 3], np.int32))
    if entry == "track":
        # two tracks; the second starts from a pose that is not finite: every row of it is -1
        init = np.stack((tref.compose(poses[0], tref.se2(0.01, 0.1, -0.1)), np.full(4, np.nan)))
        return (centers, lab, poses, init, lm["center"], lm["label"]), dict(lm_use=use, starts=np.array([0, Q - 2], np.int32),
                                                                            radii=(2.0, 0.75), n_reacquire=1, iters=3)
    if entry == "relocalize":
        q = 3
        cen, l = centers[:q].copy(), lab[:q].copy()
        l[1] = -1                                                    # a scan of padding alone: no hypothesis
        return (cen, l, lm["center"], lm["label"], use), dict(radii=(2.0, 0.75), max_hyp=300, iters=3)
    raise KeyError(entry)


@functools.lru_cache(maxsize=None)
def reference(entry, size):
    args, kw = case(entry, size)
    fn = {"map": lref.landmark_map, "refine": rref.refine, "align": aref.align, "update": uref.update, "persist": pref.persist,
          "track": tref.track, "relocalize": rlref.relocalize, "posegraph": pgref.optimize}.get(entry)
    return mref.run(args[0]) if entry == "merge" else fn(*args, **kw)


def workspace_bytes(entry, size):
    args, kw = case(entry, size)
    if entry == "merge":
        return mref.workspace_bytes(len(args[0]["a"]["label"]), len(args[0]["b"]["label"]))
    if entry == "posegraph":
        from sg_pr_amd import posegraph
        return posegraph.workspace_bytes(args[0].shape[0], args[1].size)
    Q, N = np.asarray(args[1]).shape
    if entry == "map":
        return lref.workspace_bytes(Q, N)
    if entry == "refine":
        return rref.workspace_bytes(Q, N, args[3].size)
    if entry == "align":
        return aref.workspace_bytes(Q, N, args[4].size)
    if entry in ("update", "persist"):
        return (uref if entry == "update" else pref).workspace_bytes(Q, N, len(args[4]["label"]))
    if entry == "track":
        return tref.workspace_bytes(Q, N, args[5].size, len(kw["radii"]))
    return rlref.workspace_bytes(Q, N, args[3].size, len(kw["radii"]))


# ------------------------------------------------------------------ one device call against the reference's outputs
def equal(got, want, sizes, out_fill):
    for name, n in sizes:
        assert got[name][:n].tobytes() == np.ascontiguousarray(want[name]).tobytes(), (name, got[name][:n], np.asarray(want[name]).reshape(-1))
        assert (got[name][n:].view(np.uint8) == out_fill).all(), name + ": written past the output"


def run(entry, args, kw, want, tails=True, **how):
    """the device call on (args, kw) with how = ws_fill / out_fill / workspace / stream; its outputs equal `want`.  tails:
    the case must leave record rows unwritten (map, merge)"""
    out_fill = how.get("out_fill", 0xFF)
    if entry == "map":
        got = t_map.device_map(*args, **kw, **how)
        assert got["num"].tolist() == want["num"].tolist()
        assert got["node_landmark"].tobytes() == want["node_landmark"].tobytes()
        k = want["label"].shape[0]
        assert k == want["num"][0] and (k < got["label"].shape[0] or not tails)     # unwritten tail rows exist
        for name in RECORD:
            assert got[name][:k].tobytes() == want[name].tobytes(), name
            assert (got[name][k:].view(np.uint8) == out_fill).all(), name + ": written past the records"
    elif entry == "refine":
        got = t_refine.device_refine(*args, **kw, **how)
        G, T = args[1].shape[0], kw["iters"]
        assert got["info"][:4].tolist() == want["info"].tolist()
        equal(got, want, (("poses", 4 * G), ("cost", T + 1), ("info", 4)), out_fill)
    elif entry == "align":
        t_align.same(t_align.device_align(*args, **kw, **how), want, *args[1].shape, out_fill=out_fill)
    elif entry == "update":
        got, cap = t_update.device_update(*args, **kw, **how)
        t_update.same(got, want, cap, *args[1].shape, out_fill=out_fill)
    elif entry == "persist":
        got, sizes = t_persist.device_persist(*args, **kw, **how)
        equal(got, want, [(name, sizes[name]) for name in pref.OUTPUTS], out_fill)
    elif entry == "track":
        t_track.same(t_track.device_track(*args, **kw, **how), want, *args[1].shape, out_fill=out_fill)
    elif entry == "relocalize":
        t_reloc.same(t_reloc.device_relocalize(*args, **kw, **how), want, *args[1].shape, out_fill=out_fill)
    elif entry == "merge":
        stream = how.pop("stream", None)
        ran = t_merge.launch(args[0], stream=stream, **how)
        got = {k: v.cpu().numpy() for k, v in ran["out"].items()}                 # (synchronises)
        got["sessions"] = got["sessions"].view(np.uint64)
        rows = int(want["num"][0])
        assert rows < ran["cap"] or not tails                                      # unwritten tail rows exist
        equal(got, want, [(name, (3 if name == "center" else 1) * rows) for name in RECORD] + [("old_to_new", ran["T"]), ("num", 4)],
              out_fill)
    else:
        got = t_pg.device_optimize(*args, **kw, **how)
        t_pg.same_outputs(got, want, args[0].shape[0], out_fill=out_fill)


def random_bytes(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (max(n, 16),), generator=g, dtype=torch.uint8, device="cuda")


def how_of(entry, size, ws_fill, out_fill, seed=1):
    if ws_fill == "random":
        return dict(workspace=random_bytes(workspace_bytes(entry, size), seed), out_fill=out_fill)
    return dict(ws_fill=ws_fill, out_fill=out_fill)


# ------------------------------------------------------------------ b. the references hold what a prefill could fake (CPU)
def test_reference_holds_the_values_a_prefill_could_fake():
    for size in SIZES:
        Q, N, L = SHAPE[size]
        want = reference("map", size)
        assert (want["node_landmark"] == -1).any() and (want["node_landmark"] >= 0).any() and 0 < want["num"][0] < Q * N
        assert lref.workspace_bytes(Q, N) == workspace_bytes("map", size)
        for entry in ("align", "track"):
            nl = reference(entry, size)["node_landmark"]
            assert (nl == -1).any() and (nl == -2).any() and (nl >= 0).any(), entry
            assert any((row == -1).all() for row in nl) and any((row >= 0).any() for row in nl), entry
        assert (reference("align", size)["node_landmark"][1] == -1).all()                          # the pose that is not finite
        want = reference("track", size)
        assert (want["node_landmark"][Q - 2:] == -1).all() and want["num"][0] >= 2                 # tracked scans exist
        want = reference("update", size)
        nl = want["node_landmark"]
        assert (nl == -1).any() and (nl >= L).any() and ((nl >= 0) & (nl < L)).any()
        assert want["num"][0] > L and want["num"][3] > 0 and want["num"][0] < L + Q * N             # new landmarks; tail rows
        want = reference("relocalize", size)
        flags = want["stat"][:, 5]
        assert ((flags & rlref.FOUND) != 0).any() and (flags[1] & rlref.NO_HYPOTHESIS) != 0
        assert want["win"][1].tolist() == [-1] * 4 and (want["node_landmark"][1] == -1).all()
        found = np.nonzero((flags & rlref.FOUND) != 0)[0][0]
        nl = want["node_landmark"][found]
        assert (nl == -1).any() and (nl == -2).any() and (nl >= 0).any()
        want = reference("merge", size)
        T = want["old_to_new"].size
        assert (want["old_to_new"] == -1).any() and 0 < want["num"][0] < T and want["num"][3] > 0
        want = reference("persist", size)
        assert want["num"][0] > 0 and (want["keep"] == 0).any() and (want["keep"] == 1).any()
        assert not np.isfinite(case("persist", size)[0][2]).all()                                   # a pose that is not finite
        want = reference("refine", size)
        assert want["info"][2] > 0
        want = reference("posegraph", size)
        assert want[1][0] == 0 and want[1][1] > 0 and want[1][5] > 0                                # solved, with closures
    # the two sizes carve different tables
    assert [aref.workspace_bytes(*SHAPE[s]) for s in SIZES] == [workspace_bytes("align", s) for s in SIZES]
    assert workspace_bytes("align", "small") < workspace_bytes("align", "large")


# ------------------------------------------------------------------ a. fills
def entry_id(entry):
    return "landmark_map" if entry == "map" else entry            # (a -k selection by "map" would take the whole file)


@gpu
@pytest.mark.parametrize("ws_fill", WS_FILLS, ids=lambda f: f if isinstance(f, str) else "ws%02X" % f)
@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_fills(entry, ws_fill):
    for size in SIZES:
        args, kw = case(entry, size)
        for out_fill in OUT_FILLS:
            run(entry, args, kw, reference(entry, size), **how_of(entry, size, ws_fill, out_fill))


# ------------------------------------------------------------------ c. the leftovers of a larger map
@gpu
@pytest.mark.parametrize("entry", TABLED, ids=entry_id)
def test_small_map_on_the_leftovers_of_a_large_one(entry):
    ws = random_bytes(workspace_bytes(entry, "large"), 2)
    assert workspace_bytes(entry, "small") <= ws.numel()
    for size in ("large", "small", "large"):
        args, kw = case(entry, size)
        run(entry, args, kw, reference(entry, size), workspace=ws, out_fill=0x5A)


# ------------------------------------------------------------------ d. one arena, the pipeline's chain
@functools.lru_cache(maxsize=None)
def chain():
    """the pipeline on a planted world of 3 drives of 12 scans, in NumPy: a list of (entry, args, kw, want, bytes).  A
    step takes the outputs of the steps before it where place_db does; the device chain is handed the same arrays only
    after its own outputs were found equal to them to the bit."""
    from sg_pr_amd import synth
    S = 12
    w = synth.landmark_world(3, scans=S)
    N = w["labels"].shape[1]
    first, last = slice(0, 2 * S), slice(2 * S, 3 * S)
    steps = []

    def step(entry, args, kw, fn, need):
        want = fn(*args, **kw)
        steps.append((entry, args, kw, want, need))
        return want

    cen, lab = w["centers"][first], w["labels"][first]
    kw = dict(starts=w["starts"][:2])
    lm = step("map", (cen, lab, w["odom"][first]), kw, lref.landmark_map, lref.workspace_bytes(2 * S, N))
    L = int(lm["num"][0])
    use = (lm["count"] >= 2).astype(np.uint8)
    fixed = np.zeros(2 * S, np.uint8)
    fixed[0] = 1
    rf = step("refine", (cen, lm["node_landmark"], w["odom"][first], use), dict(fixed=fixed, iters=3), rref.refine,
              rref.workspace_bytes(2 * S, N, L))
    cen2, lab2 = w["centers"][last], w["labels"][last]
    start = synth._se2_compose(w["truth"][last], tref.se2(0.01, 0.2, -0.1)[None])
    al = step("align", (cen2, lab2, start, lm["center"], lm["label"]), dict(lm_use=use, radius=2.0, iters=3), aref.align,
              aref.workspace_bytes(S, N, L))
    rec = {k: lm[k] for k in RECORD}
    up = step("update", (cen2, lab2, al["poses"], al["node_landmark"], rec), dict(session_base=2), uref.update,
              uref.workspace_bytes(S, N, L))
    L2 = int(up["num"][0])
    ps = step("persist", (cen2, lab2, al["poses"], al["node_landmark"], {"center": lm["center"], "label": lm["label"], "use": use}),
              dict(min_expected=2, max_seen_ratio=0.5), pref.persist, pref.workspace_bytes(S, N, L))
    keep = np.concatenate((ps["keep"], np.ones(L2 - L, np.uint8)))
    init = synth._se2_compose(w["truth"][last][:1], tref.se2(0.02, 0.3, 0.2)[None])
    tr = step("track", (cen2, lab2, w["odom"][last], init, up["center"], up["label"]),
              dict(lm_use=keep, radii=(8.0, 2.0, 0.75), n_reacquire=1, iters=3), tref.track, tref.workspace_bytes(S, N, L2, 3))
    step("relocalize", (cen2[::5], lab2[::5], up["center"], up["label"], keep), dict(radii=(2.0, 0.75), max_hyp=300, iters=3),
         rlref.relocalize, rlref.workspace_bytes(len(cen2[::5]), N, L2, 2))
    compact = {"a": {k: up[k] for k in RECORD}, "b": mref.lm_of(np.zeros((0, 3)), []), "kw": {"keep_a": keep}}
    step("merge", (compact,), {}, lambda c: mref.run(c), mref.workspace_bytes(L2, 0))
    X = np.concatenate((rf["poses"], tr["poses"]))
    rows, cols = w["rows"], w["cols"]
    ok = (rows < 3 * S) & (cols < 3 * S)
    rows, cols = rows[ok][:40], cols[ok][:40]
    T = np.ascontiguousarray(synth._se2_compose(synth._se2_inverse(w["truth"][cols]), w["truth"][rows]))
    step("posegraph", (X, rows, cols, T), dict(starts=w["starts"], max_iters=40), pgref.optimize, None)
    return steps


@gpu
def test_one_arena_through_the_pipeline_twice():
    from sg_pr_amd import posegraph
    steps = chain()
    need = [n if n is not None else posegraph.workspace_bytes(a[0].shape[0], a[1].size) for _, a, _, _, n in steps]
    arena = random_bytes(max(need), 3)
    for _ in range(2):                                           # the second pass runs on what the first left behind
        for entry, args, kw, want, _ in steps:
            run(entry, args, kw, want, tails=False, workspace=arena, out_fill=0x5A)


def test_the_chain_is_not_trivial():
    """(CPU) every step of the reference chain does something: landmarks, refits, matches, new landmarks, retirements,
    tracked scans, a scan found, records dropped, a solve"""
    got = {entry: want for entry, _, _, want, _ in chain()}
    assert got["map"]["num"][0] > 50 and got["refine"]["info"][2] > 0
    assert (got["align"]["stat"][:, 0] > 10).all() and (got["align"]["node_landmark"] == -2).any()
    assert got["update"]["num"][3] > 0 and got["update"]["num"][2] > 0
    assert got["persist"]["num"][0] > 0 and got["track"]["num"][0] > 0
    assert ((got["relocalize"]["stat"][:, 5] & rlref.FOUND) != 0).any()
    assert got["merge"]["num"][1] == got["persist"]["num"][0] and got["merge"]["num"][0] > 0
    assert got["posegraph"][1][0] == 0 and got["posegraph"][1][5] > 0


# ------------------------------------------------------------------ e. two streams, two inputs, two fills
@gpu
@pytest.mark.parametrize("entry", ["align", "track", "relocalize"])
def test_two_streams_two_inputs_two_fills(entry):
    """the small case on a 0x00 workspace and the large one on random bytes, launched from two threads at one moment on
    two streams.  Both workspaces are made here, before the threads start and under the synchronize() below; the inputs
    and the output prefills are made by the helpers inside the threads, on the null stream, and each helper has its side
    stream wait for the null stream before the call - without that nothing would order a fill before the call's own table
    clear on a non-blocking stream"""
    ws = torch.zeros(max(workspace_bytes(entry, "small"), 16), dtype=torch.uint8, device="cuda")
    hows = [dict(workspace=ws, out_fill=0x5A, stream=torch.cuda.Stream()),
            dict(workspace=random_bytes(workspace_bytes(entry, "large"), 4), out_fill=0xFF, stream=torch.cuda.Stream())]
    for size in SIZES:
        reference(entry, size)
    torch.cuda.synchronize()
    gate, errors = threading.Barrier(2), []

    def work(size, how):
        try:
            args, kw = case(entry, size)
            gate.wait(timeout=60)
            run(entry, args, kw, reference(entry, size), **how)
        except BaseException as e:                               # noqa: B902 (reported by the test's thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(size, how)) for size, how in zip(SIZES, hows)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]

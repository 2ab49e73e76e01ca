"""sgpr_score_mine / sgpr_mine_rows off the GPU: the exported symbols, the host-side argument checks (no device is touched)
and the workspace bound.  CPU only."""
import ctypes
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _zeroed_handle():
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    return zeroed, ctypes.cast(zeroed, ctypes.c_void_p)


def test_exported_symbols_and_flags():
    import os
    from sg_pr_amd import engine
    lib = engine.load_library()
    for sym in ("sgpr_score_mine_workspace_bytes", "sgpr_score_mine", "sgpr_mine_rows_workspace_bytes", "sgpr_mine_rows"):
        assert sym in engine.ABI_SYMBOLS
        getattr(lib, sym)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgpr.h")) as f:
        h = f.read()
    assert "#define SGPR_MINE_NEGATIVES 2" in h and "#define SGPR_MINE_POSITIVES 4" in h
    assert engine.Engine.MINE_NEGATIVES == 2 and engine.Engine.MINE_POSITIVES == 4
    assert lib.sgpr_abi_version() == 11


def test_argument_checks_touch_no_device():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every failing call fails its host-side checks
    R, M = 100, 300
    need = lib.sgpr_score_mine_workspace_bytes(h, R, M, 4, 2)
    assert need > 0

    def fused(h=h, rows=p, cols=p, pose=p, vals=p, idx=p, flags=2, k=4, dp=3.0, dn=20.0, ws=p, wb=need, r=R, row0=0):
        return lib.sgpr_score_mine(h, rows, r, cols, M, pose, None, None, row0, 10, flags, dp, dn, k, vals, idx, ws, wb,
                                   None)

    def matrix(h=h, score=p, pose=p, vals=p, idx=p, flags=2, k=4, dp=3.0, dn=20.0, ld=M, r=R, row0=0):
        return lib.sgpr_mine_rows(h, score, r, M, ld, pose, None, None, row0, 10, flags, dp, dn, k, vals, idx, None, 0,
                                  None)

    for call in (fused, matrix):
        assert call(h=None) == -1
        assert call(pose=None) == -1 and b"NULL" in lib.sgpr_last_error()
        assert call(vals=None) == -1 and call(idx=None) == -1
        for k in (0, 17, -3):
            assert call(k=k) == -1 and b"k must" in lib.sgpr_last_error()
        for flags in (0, 1, 2 | 4, 2 | 8, 4 | 16, -1):
            assert call(flags=flags) == -1 and b"flags" in lib.sgpr_last_error(), flags
        assert call(dp=float("nan")) == -1 and call(dn=float("nan")) == -1
        assert call(dp=20.5) == -1 and b"d_pos" in lib.sgpr_last_error()
        assert call(dp=-1.0) == -1 and call(dp=-1.0, dn=-0.5) == -1
        assert call(row0=0x7fffffff - R + 1) == -1 and b"row0" in lib.sgpr_last_error()
        assert call(r=0, row0=0x7fffffff) == 0       # an empty query set needs nothing
    assert fused(rows=None) == -1 and fused(cols=None) == -1
    assert fused(wb=need - 1) == -7 and b"workspace" in lib.sgpr_last_error()
    assert fused(ws=None) == -7
    assert matrix(score=None) == -1 and matrix(ld=M - 1) == -1
    assert lib.sgpr_score_mine_workspace_bytes(h, R, M, 17, 2) == 0
    assert lib.sgpr_score_mine_workspace_bytes(h, R, M, 4, 6) == 0
    assert lib.sgpr_score_mine_workspace_bytes(h, R, M, 4, 0) == 0
    assert lib.sgpr_mine_rows_workspace_bytes(h, R, M, 4, 2) == 0


def test_workspace_grows_with_r_plus_m():
    from sg_pr_amd import engine
    lib = engine.load_library()
    keep, h = _zeroed_handle()
    n = 100000
    for k in (1, 16):
        for flags in (2, 4, 2 | 1, 4 | 1):
            ws = lib.sgpr_score_mine_workspace_bytes(h, n, n, k, flags)
            assert 0 < ws < 0.01 * 4 * n * n, ws
            # twice the rows: the workspace grows with R (operands, row poses), not with R * M
            ws2 = lib.sgpr_score_mine_workspace_bytes(h, 2 * n, n, k, flags)
            assert ws2 - ws < 0.01 * 4 * n * n
            assert ws >= lib.sgpr_score_topk_workspace_bytes(h, n, n, k, flags & 1)


# ---------------------------------------------------------------------------------------------------- training side
def test_mined_pair_assembly():
    import numpy as np
    from sg_pr_amd.train import PairSet, mined_pairs
    # two sequences: graphs 0..4 (members [0, 2, 4]) and 5..8 (members [5, 6, 8]); local indices, -1 = empty slot
    g0 = (np.array([0, 2, 4]), np.array([[2, 1], [0, -1], [0, 1]]))       # (0,4) (0,2) (2,0)dup (4,0)dup (4,2)
    g1 = (np.array([5, 6, 8]), np.array([[2, -1], [-1, -1], [0, 1]]))     # (5,8) (8,5)dup (8,6)
    base = np.array([[2, 0], [6, 7]])                                     # (0,2) is known, in the other order
    got = mined_pairs([g0, g1], base)
    assert got.dtype == np.int64
    assert got.tolist() == [[0, 4], [2, 4], [5, 8], [6, 8]]
    # within one sequence only: no pair mixes the two member sets
    for a, b in got:
        assert (a < 5) == (b < 5)
    assert mined_pairs([], base).shape == (0, 2)
    assert mined_pairs([(np.array([3]), np.array([[-1, -1]]))], base).shape == (0, 2)
    # targets: the mining thresholds are target_of's, so the rule never reaches its exit
    xz = np.array([[0.0, 0.0], [0.0, 1.0], [2.0, 2.0], [0.0, 0.0], [30.0, 0.0]])
    pairs = np.array([[0, 2], [0, 4], [1, 4]])
    assert PairSet._targets(xz, pairs, 3.0).tolist() == [1.0, 0.0, 0.0]


def test_pairset_sequence_from_files(tmp_path):
    import numpy as np
    from sg_pr_amd.parser_sg import sgpr_args
    from sg_pr_amd.train import PairSet
    golden = os.path.join(REPO, "tests", "golden", "data")
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / "00.txt").write_text("0.json 3.json\n0.json 250.json\n")
    (lists / "08.txt").write_text("250.json 3.json\n")
    (lists / "05.txt").write_text("3.json 0.json\n")
    a = sgpr_args()
    a.pair_list_dir, a.graph_pairs_dir = str(lists), golden
    a.train_sequences, a.eval_sequences = ["00", "05"], ["08"]
    data = PairSet.from_files(a)
    # graphs 0.json, 3.json, 250.json all first appear in sequence 00's list
    assert data.sequence.tolist() == [0, 0, 0]
    a.train_sequences, a.eval_sequences = ["08"], ["00"]
    data = PairSet.from_files(a)
    assert data.sequence.tolist() == [0, 0, 1]            # 250, 3 from 08; 0 from 00
    assert data.train_pairs.tolist() == [[0, 1]] and data.eval_pairs.tolist() == [[2, 1], [2, 0]]
    assert data.xz.shape == (3, 2) and data.p_thresh == 3.0
    poses = np.zeros((2, 12))
    assert PairSet(np.zeros((2, 4, 3)), -np.ones((2, 4)), poses, [[0, 1]], []).sequence is None
    import pytest
    with pytest.raises(ValueError):
        PairSet(np.zeros((2, 4, 3)), -np.ones((2, 4)), poses, [[0, 1]], [], sequence=[0])


def test_cli_parsing_of_the_mining_flags():
    import pytest
    from sg_pr_amd.train import parse_cli
    ns = parse_cli(["cfg.yml", "--hard-negatives", "4", "--hard-positives", "2", "--mine-every", "3"])
    assert (ns.hard_negatives, ns.hard_positives, ns.mine_every) == (4, 2, 3)
    ns = parse_cli([])
    assert (ns.hard_negatives, ns.hard_positives, ns.mine_every) == (0, 0, 2)
    with pytest.raises(SystemExit):
        parse_cli(["--hard-negatives", "x"])


def test_place_db_cli_has_hard():
    import inspect
    from sg_pr_amd import place_db
    assert "--hard" in inspect.getsource(place_db.main)
    assert callable(place_db.hard_pairs_of) and hasattr(place_db.PlaceDatabase, "query_ids_hard")

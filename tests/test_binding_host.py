"""The Python binding follows include/sgpr.h and nothing else (no GPU): the header parser on a literal text, the ctypes
signatures it gives the loaded library - a set of functions that together use every parameter and return type of the
header, written out here as literals -, every declared function bound, and the limits / flag bits / error codes the
binding mirrors pinned to their values.  Last, the one session-table check behind the entry points of all four headers:
the same bad table gets the same answer from each."""
import ctypes
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

vp, i32, i64, sz, f32, dbl = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float,
                              ctypes.c_double)

TEXT = """
#ifndef DEMO_H
#define DEMO_H
#include <stddef.h>
#define SGPR_DEMO_LIMIT 48
#define SGPR_DEMO_MASK 0x10
#define SGPR_DEMO_TEXT "not a number"
#ifdef __cplusplus
extern "C" {
#endif
enum {
    SGPR_OK = 0,
    SGPR_E_DEMO = -3   /* a comment; with a semicolon */
};
typedef struct sgpr_handle sgpr_handle;
typedef struct sgpr_thing {
    int32_t a;   /* fields; are; skipped */
    float b[4];
} sgpr_thing;
/* int sgpr_commented_out(int x); */
int sgpr_first(const sgpr_handle* h, const float* d_x, int n, int64_t ld,   // trailing; comment
               size_t bytes, float scale,
               double tol, sgpr_thing** out, void* stream);
size_t sgpr_second(void);
const char* sgpr_third(void);
void sgpr_fourth(sgpr_handle* h EXTRA);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_the_style_of_the_header():
    from sg_pr_amd import _build
    abi = _build.parse_header(TEXT.replace(" EXTRA", ""))
    assert abi.functions == [("sgpr_first", i32, [vp, vp, i32, i64, sz, f32, dbl, vp, vp]),
                             ("sgpr_second", sz, []), ("sgpr_third", ctypes.c_char_p, []), ("sgpr_fourth", None, [vp])]
    assert abi.constants == {"SGPR_DEMO_LIMIT": 48, "SGPR_DEMO_MASK": 16}
    assert abi.errors == {"SGPR_OK": 0, "SGPR_E_DEMO": -3}


@pytest.mark.parametrize("extra,named", [(", long double x", "long double x"), (", sgpr_thing by_value", "sgpr_thing by_value"),
                                         (", unsigned flags", "unsigned flags")])
def test_parser_refuses_a_type_it_cannot_bind(extra, named):
    """never ctypes' implicit int: the error names the declaration and the parameter"""
    from sg_pr_amd import _build
    with pytest.raises(ImportError) as err:
        _build.parse_header(TEXT.replace(" EXTRA", extra))
    assert "sgpr_fourth" in str(err.value) and named in str(err.value)


def test_parser_refuses_a_return_type_it_cannot_bind():
    from sg_pr_amd import _build
    with pytest.raises(ImportError, match="sgpr_second"):
        _build.parse_header(TEXT.replace(" EXTRA", "").replace("size_t sgpr_second", "long sgpr_second"))


PINNED = {
    "sgpr_create": (i32, [vp, sz, vp, i32, vp]),
    "sgpr_destroy": (None, [vp]),
    "sgpr_last_error": (ctypes.c_char_p, []),
    "sgpr_pair_plan_ints": (sz, [i64, i32]),
    "sgpr_pair_plan": (i32, [vp, vp, i64, i32, i32, vp, sz, vp, vp, vp]),
    "sgpr_embed_ragged": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, sz, vp]),
    "sgpr_score_all_pairs_multi": (i32, [vp, i32, vp, vp, sz, vp]),
    "sgpr_pair_threshold_counts": (i32, [vp, vp, i32, i32, i64, i32, vp, dbl, dbl, vp, i64, vp, i32, vp, i32, vp, vp, vp,
                                         sz, vp]),
    "sgpr_verify_pairs": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, vp, i64, f32, f32, f32, f32, i32, vp, vp]),
    "sgpr_closure_consistency": (i32, [vp, vp, vp, i32, vp, i32, vp, i32, vp, i32, dbl, dbl, dbl, vp, vp, vp, sz, vp]),
    "sgpr_score_session_above": (i32, [vp, vp, i32, vp, i32, i32, vp, i32, i32, i32, i32, vp, i32, vp, i32, vp, i32, i32,
                                       f32, vp, vp, vp, vp, i64, vp, vp, vp, sz, vp]),
}


def test_signatures_of_the_real_header_are_the_pinned_ones():
    from sg_pr_amd import _build, engine
    lib = engine.load_library()
    parsed = {name: (restype, argtypes) for name, restype, argtypes in _build.header_abi().functions}
    for name, (restype, argtypes) in PINNED.items():
        assert parsed[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # together they use every type the header has
    used = {t for restype, argtypes in PINNED.values() for t in [restype] + argtypes}
    assert used == {t for restype, argtypes in parsed.values() for t in [restype] + argtypes}
    assert used == {None, ctypes.c_char_p, vp, i32, i64, sz, f32, dbl}


def test_every_declared_function_is_bound():
    from sg_pr_amd import _build, engine
    lib = engine.load_library()
    functions = _build.header_abi().functions
    assert len(functions) == 100 == len(engine.ABI_SYMBOLS) == len(set(engine.ABI_SYMBOLS))
    assert [name for name, _, _ in functions] == engine.ABI_SYMBOLS
    for name, restype, argtypes in functions:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name      # (None: never set)
        assert fn.restype is restype, name                                         # (ctypes' default is c_int)


def test_mirrored_constants_have_the_header_values():
    from sg_pr_amd import engine
    E = engine.Engine
    assert (E.TOPK_CAUSAL, E.TOPK_LARGE_MAX, E.SEQ_FORWARD, E.SEQ_REVERSE, E.SEQ_MAX_LEN) == (1, 4096, 2, 4, 32)
    assert (E.SEQ_MAX_PATHS, E.SEQ_PATH_MAX_OFFSET, E.SESSION_MAX) == (16, 64, 64)
    assert (engine.SEQ_MAX_PATHS, engine.SEQ_PATH_MAX_OFFSET, engine.SESSION_MAX) == (16, 64, 64)
    assert (E.PEAK_MAX_RADIUS, E.PEAK_STRIP, E.MINE_NEGATIVES, E.MINE_POSITIVES) == (1024, 1024, 2, 4)
    assert (E.MAX_POOLED_THRESHOLDS, E.MAX_PAIR_JOBS, engine.MAX_NODES) == (2047, 8, 256)
    assert (engine.VERIFY_MAX_NODES, engine.VERIFY_INVALID_INDEX, engine.VERIFY_NO_HYPOTHESIS, engine.VERIFY_TRUNCATED,
            engine.VERIFY_NONFINITE) == (256, 1, 2, 4, 8)
    assert (engine.CONSISTENCY_MAX_CLOSURES, engine.CONSISTENCY_MAX_GROUPS) == (16384, 4096)
    assert engine.SGPR_OK == 0
    assert engine.ERROR_NAMES == {-1: "SGPR_E_INVALID", -2: "SGPR_E_DIMS", -3: "SGPR_E_NODES", -4: "SGPR_E_K",
                                  -5: "SGPR_E_LABEL", -6: "SGPR_E_HIP", -7: "SGPR_E_WORKSPACE", -8: "SGPR_E_BLOB"}
    assert all(isinstance(v, int) for v in (E.TOPK_CAUSAL, engine.MAX_NODES, engine.VERIFY_NONFINITE))


# (table or None, n or None = its length, limit, a word of the message) - every fault of a session table
BAD_SESSION_TABLES = {
    "null_with_n_2": (None, 2, 8, "NULL"),
    "table_with_n_0": ([0, 4], 0, 8, "with n = 0"),
    "n_minus_1": ([0, 4], -1, 8, "0..64"),
    "n_65": ([0] * 65, 65, 8, "0..64"),
    "first_entry_1": ([1, 4], None, 8, "start at 0"),
    "decreasing": ([0, 5, 4], None, 8, "decreasing entry at 2"),
    "past_the_limit": ([0, 4, 9], None, 8, "past 8"),
    "limit_0": ([0, 1], None, 0, "past 0"),
}


@pytest.mark.parametrize("case", sorted(BAD_SESSION_TABLES))
def test_one_session_table_check_behind_every_header(case):
    """sgpr_session_filter (its row table), sgpr_posegraph_optimize, sgpr_localize_scans and sgpr_landmark_map refuse a
    bad session table with the same code and, after the function's name and apart from the word "row", the same text.
    Wild device pointers: had the device been touched, the call would have failed otherwise or crashed."""
    from sg_pr_amd import engine, landmarks, localize, posegraph
    lib = engine.load_library()
    assert posegraph.load_library() is lib and localize.load_library() is lib and landmarks.load_library() is lib
    values, n, limit, word = BAD_SESSION_TABLES[case]
    table = None if values is None else np.ascontiguousarray(values, dtype=np.int32)
    t = None if table is None else ctypes.c_void_p(table.ctypes.data)
    n = len(values) if n is None else n
    g = ctypes.c_void_p(0xdead0000)                 # never dereferenced
    zeroed = ctypes.create_string_buffer(1 << 16)   # a zeroed handle: plain fields only, no device state behind it
    radius = np.full(12, 0.75)
    calls = {
        "sgpr_session_filter": lambda: lib.sgpr_session_filter(
            ctypes.cast(zeroed, ctypes.c_void_p), g, limit, 300, 300, 0, 8, 2, None, 0, t, n, None, 0, None, 0, -1, g, 300,
            None, None),
        "sgpr_posegraph_optimize": lambda: lib.sgpr_posegraph_optimize(
            g, limit, t, n, g, g, g, None, 5, None, 1.0, 1.0, 1.0, 1.0, 10, 1e-9, g, g, g, g, 1 << 40, None),
        "sgpr_localize_scans": lambda: lib.sgpr_localize_scans(
            g, 20, g, g, g, limit, 4, g, t, n, 2, 1.0, 0.9, g, g, g, None),
        "sgpr_landmark_map": lambda: lib.sgpr_landmark_map(
            g, g, limit, 10, g, t, n, radius.ctypes.data, 12, 0.75, 80, g, g, g, g, g, g, g, g, g, 1 << 40, None),
    }
    texts = {}
    for fn, call in calls.items():
        assert call() == -1, fn                      # SGPR_E_INVALID
        message = lib.sgpr_last_error().decode()
        assert message.startswith(fn + ": "), message
        texts[fn] = message[len(fn) + 2:]
    row = texts.pop("sgpr_session_filter")
    assert word in row and "row " in row and "  " not in row, row
    for fn, text in texts.items():
        assert text == row.replace("row ", "", 1), (fn, text, row)
        assert "  " not in text and word in text, (fn, text)

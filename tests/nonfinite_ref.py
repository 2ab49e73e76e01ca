"""What a scoring kernel owes a pair whose pooled vectors are not all finite, from the float64 tail of tests/score_ref.py.
TEST INFRASTRUCTURE: used by tests/, never by the product.

A NaN pooled vector is the library's own error marker (include/sgpr.h: a graph that breaks its node promise), and every
consumer's "a NaN score never qualifies" rests on it reaching the score.  Class of a (row graph, column graph) pair:

  MUST_NAN   a NaN anywhere in either vector: the score is NaN, in whatever order a kernel sums (NaN op x = NaN; the
             reference's np.maximum ReLUs hand it on, so its own score is NaN too - asserted here)
  INF_BOUND  no NaN but a +-inf in either vector, and the float64 score is not NaN: the kernel's score is NaN or within
             the bar of the reference.  One-sided: where infinite terms of both signs meet depends on the order of the
             sums, and a kernel may associate differently from the reference
  INF_FREE   the same, and the float64 score is NaN: no value is owed (only the bit contracts between entry points hold)
  FINITE     both vectors finite: within the bar of the reference, like any other input"""
import numpy as np

import score_ref

FINITE, MUST_NAN, INF_BOUND, INF_FREE = 0, 1, 2, 3

QNAN_POS = 0x7FC00000        # the marker the embed kernels write
QNAN_NEG = 0xFFC00000        # the same with the sign bit set (an integer-max ReLU would turn it into 0)


def plant_bits(a, index, bits):
    """a[index] = the float32 with exactly these bits, written through an integer view (no arithmetic that could
    canonicalise a NaN); a: float32 array, modified in place."""
    assert a.dtype == np.float32 and a.flags.c_contiguous
    a.view(np.uint32)[index] = np.uint32(bits)
    return a


def classes(sd, rows, cols):
    """-> (cls int8 [R, M], ref): the class of every pair and score_ref.tail's dict on the same inputs."""
    rows, cols = np.asarray(rows, dtype=np.float32), np.asarray(cols, dtype=np.float32)
    with np.errstate(all="ignore"):
        ref = score_ref.tail(sd, rows, cols)
    rnan, cnan = np.isnan(rows).any(axis=1), np.isnan(cols).any(axis=1)
    rinf, cinf = np.isinf(rows).any(axis=1), np.isinf(cols).any(axis=1)
    nan = rnan[:, None] | cnan[None, :]
    inf = (rinf[:, None] | cinf[None, :]) & ~nan
    ref_nan = np.isnan(ref["score"])
    cls = np.full(nan.shape, FINITE, dtype=np.int8)
    cls[inf & ~ref_nan] = INF_BOUND
    cls[inf & ref_nan] = INF_FREE
    cls[nan] = MUST_NAN
    assert ref_nan[nan].all(), "the float64 reference lost a NaN"
    assert not ref_nan[cls == FINITE].any(), "the float64 reference is NaN on finite inputs"
    return cls, ref


def violations(got, cls, ref, tol):
    """got [R, M] (any float dtype) against the rule -> bool [R, M], True where it is broken.  tol [R, M]: the bar of the
    finite comparison (entries of NaN-class pairs are not read)."""
    got = np.asarray(got, dtype=np.float64)
    gnan = np.isnan(got)
    with np.errstate(invalid="ignore"):
        far = ~(np.abs(got - ref["score"]) <= tol)          # (True for a NaN on either side)
    bad = np.zeros(cls.shape, dtype=bool)
    bad |= (cls == MUST_NAN) & ~gnan
    bad |= (cls == FINITE) & far
    bad |= (cls == INF_BOUND) & ~gnan & far
    return bad


def element_indices(f):
    """first, the two middle and the last element of an f-wide vector (32: 0, 15, 16, 31 - one in each quarter a lane
    group of the tuned kernels owns; 48: 0, 23, 24, 47)"""
    return [0, f // 2 - 1, f // 2, f - 1]


def plants(rows, cols):
    """The planted inputs of tests/test_gpu_score_nonfinite.py on clean rows [R >= 37, F], cols [M >= 131, F]
    -> list of (name, rows', cols', square).  square: cols' is rows' (one array, the poisoned graphs on both sides).
    The last row and the last column (a partial tile at 37 x 131) are among the single-element plants."""
    r, m, f = rows.shape[0], cols.shape[0], rows.shape[1]
    ix = element_indices(f)
    out = []

    def fresh():
        return rows.copy(), cols.copy()

    for name, bits, pr, pc in (("NaN graphs, 7fc00000", QNAN_POS, 20, m - 1), ("NaN graphs, ffc00000", QNAN_NEG, r - 1, 64)):
        a, b = fresh()
        plant_bits(a, (pr, slice(None)), bits)
        plant_bits(b, (pc, slice(None)), bits)
        out.append((name, a, b, False))
    a, b = fresh()
    for g, i, bits in zip((2, 17, 21, r - 1), ix, (QNAN_POS, QNAN_NEG, QNAN_POS, QNAN_NEG)):
        plant_bits(a, (g, i), bits)
    out.append(("one NaN element in four rows", a, b, False))
    a, b = fresh()
    for g, i, bits in zip((0, 63, 64, m - 1), ix, (QNAN_NEG, QNAN_POS, QNAN_NEG, QNAN_POS)):
        plant_bits(b, (g, i), bits)
    out.append(("one NaN element in four columns", a, b, False))
    a, b = fresh()
    a[r - 1, ix[1]] = np.inf
    out.append(("one +inf element in a row", a, b, False))
    a, b = fresh()
    b[m - 1, ix[2]] = -np.inf
    out.append(("one -inf element in a column", a, b, False))
    a, b = fresh()
    a[7, 0], a[7, f - 1] = np.inf, -np.inf
    out.append(("+inf and -inf in one row", a, b, False))
    a, b = fresh()
    a[18] = np.inf
    out.append(("a row of +inf", a, b, False))
    a, _ = fresh()
    plant_bits(a, (r - 1, slice(None)), QNAN_POS)
    plant_bits(a, (4, ix[2]), QNAN_NEG)
    out.append(("square: NaN graphs on both sides", a, a, True))
    return out

"""The host-only weight packer (sg_pr_amd/csrc/sgpr_model.hpp) byte for byte: every buffer sgpr_create uploads and every
offset / scalar it derives, for blobs that reach every branch of the packer, against tests/golden/model_pack.json.

The golden file records what sgpr_create built BEFORE the packer was split out of it (its host vectors written to files
just ahead of their upload), so a digest here is the layout the kernels have been tested on.  No GPU: tests/pack_dump.cpp
is a stand-alone program over the header alone.
"""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO

FULL = (12, 64, 64, 32, 16, 16)
SMALL = (5, 24, 40, 16, 8, 12)              # inside the built shape: padded into it; any-shape model at its own dims
UNALIGNED = (20, 72, 100, 40, 24, 20)       # any-shape inside the wide limits, no width a multiple of 32
WIDE_LIMIT = (32, 128, 128, 64, 16, 16)     # exactly SGPR_WIDE_MAX_*
WIDE_BEYOND = (33, 128, 128, 64, 16, 16)    # one label more: no wide buffer
LARGEST = (64, 256, 256, 128, 64, 64)       # SGPR_ANY_MAX_*
FILES = ("built.bin", "generic.bin", "wide_planes.bin", "wide_tbs.bin")


def block_shapes(d):
    L, f1, f2, f3 = d[:4]
    return [(f1, 6), (f1, 2 * L), (f2, 2 * f1), (f2, 2 * f1), (f3, 2 * f2), (f3, 2 * f2), (f3, 2 * f3)]


def tail_sizes(d):
    f, t, b = d[3:]
    return [f * f, f * f * t, t * 2 * f, t, b * t, b, b, 1]


def block_offset(d, b):
    return sum(co * ci2 + 4 * co for co, ci2 in block_shapes(d)[:b])


def tail_offset(d, q):
    return block_offset(d, 7) + sum(tail_sizes(d)[:q])


def random_blob(d, seed):
    """weights with exact zeros, positive running_var and some negative gamma (a zero weight then folds to -0.0)"""
    rs = np.random.RandomState(seed)
    parts = []
    for cout, cin2 in block_shapes(d):
        w = (0.3 * rs.standard_normal((cout, cin2))).astype(np.float32)
        w[rs.random_sample(w.shape) < 0.1] = 0.0
        gamma = (rs.uniform(0.5, 1.5, cout) * np.where(rs.random_sample(cout) < 0.3, -1.0, 1.0)).astype(np.float32)
        beta = (0.1 * rs.standard_normal(cout)).astype(np.float32)
        mean = (0.1 * rs.standard_normal(cout)).astype(np.float32)
        var = rs.uniform(0.5, 2.0, cout).astype(np.float32)
        parts += [w.ravel(), gamma, beta, mean, var]
    parts += [(0.2 * rs.standard_normal(n)).astype(np.float32) for n in tail_sizes(d)]
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def shipped_blob():
    from oracle import sgpr_oracle
    from sg_pr_amd import engine
    return engine.blob_from_state_dict(sgpr_oracle.load_checkpoint(os.path.join(GOLDEN, "model.pth")))


def with_folded_weight(blob, d, b, target):
    """blob with W[0][0] of block b set so that its fold s * W is about `target`"""
    out = blob.copy()
    cout, cin2 = block_shapes(d)[b]
    at = block_offset(d, b)
    gamma, var = float(out[at + cout * cin2]), float(out[at + cout * cin2 + 3 * cout])
    out[at] = np.float32(target * np.sqrt(var + 1e-5) / gamma)
    return out


def with_head(blob, d, fc1_00, fc2):
    out = blob.copy()
    out[tail_offset(d, 4)] = fc1_00
    out[tail_offset(d, 6):tail_offset(d, 7)] = fc2
    return out


def cases():
    """name -> (dims, blob); every blob but the shipped one comes from a seeded RandomState (a frozen stream)"""
    ship = shipped_blob()
    unal = random_blob(UNALIGNED, 3)
    return {
        "shipped": (FULL, ship),
        "smaller": (SMALL, random_blob(SMALL, 2)),
        "wide_unaligned": (UNALIGNED, unal),
        "wide_at_limit": (WIDE_LIMIT, random_blob(WIDE_LIMIT, 4)),
        "wide_beyond_limit": (WIDE_BEYOND, random_blob(WIDE_BEYOND, 5)),
        "largest": (LARGEST, random_blob(LARGEST, 6)),
        "edgeconv_beyond_f16": (FULL, with_folded_weight(ship, FULL, 2, 2.0e5)),
        "wide_embed_beyond_f16": (UNALIGNED, with_folded_weight(unal, UNALIGNED, 0, 2.0e5)),
        "head_beyond_f16": (FULL, with_head(ship, FULL, 1.0e3, 1.0e3)),
        "head_zero": (FULL, with_head(ship, FULL, 1.0, 0.0)),
    }


def digest_dir(out_dir):
    """what a dump directory holds, in the golden file's form"""
    with open(os.path.join(out_dir, "meta.txt")) as f:
        meta = f.read()
    sha = {}
    for name in FILES:
        path = os.path.join(out_dir, name)
        if os.path.exists(path):
            with open(path, "rb") as f:
                sha[name] = hashlib.sha256(f.read()).hexdigest()
    return {"meta": meta, "sha256": sha}


@pytest.fixture(scope="session")
def pack_dump(tmp_path_factory):
    from sg_pr_amd import _build
    exe = str(tmp_path_factory.mktemp("pack_dump") / "pack_dump")
    subprocess.run([_build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"),
                    "-I", _build.CSRC, os.path.join(REPO, "tests", "pack_dump.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="session")
def all_cases():
    return cases()


@pytest.fixture(scope="session")
def golden():
    with open(os.path.join(GOLDEN, "model_pack.json")) as f:
        return json.load(f)


def meta_of(text):
    return dict(line.split(" ", 1) for line in text.splitlines())


CASE_NAMES = ["shipped", "smaller", "wide_unaligned", "wide_at_limit", "wide_beyond_limit", "largest",
              "edgeconv_beyond_f16", "wide_embed_beyond_f16", "head_beyond_f16", "head_zero"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_packer_reproduces_the_recorded_layouts(name, pack_dump, all_cases, golden, tmp_path):
    dims, blob = all_cases[name]
    blob.tofile(str(tmp_path / "blob.bin"))
    subprocess.run([pack_dump, str(tmp_path / "blob.bin")] + [str(v) for v in dims] + [str(tmp_path)], check=True)
    got = digest_dir(str(tmp_path))
    want = golden[name]
    assert got["meta"].splitlines() == want["meta"].splitlines()
    assert got["sha256"] == want["sha256"]


def test_cases_reach_the_branches_they_are_named_for(all_cases, golden):
    """the recorded layouts themselves: which buffers exist and which range flags fell, per case"""
    assert sorted(all_cases) == sorted(CASE_NAMES) == sorted(golden)
    files = {n: sorted(golden[n]["sha256"]) for n in CASE_NAMES}
    meta = {n: meta_of(golden[n]["meta"]) for n in CASE_NAMES}
    for n in ("shipped", "smaller", "edgeconv_beyond_f16", "head_beyond_f16", "head_zero"):
        assert files[n] == ["built.bin", "generic.bin"] and meta[n]["wide.ok"] == "0"
    for n in ("wide_unaligned", "wide_at_limit"):
        assert files[n] == ["generic.bin", "wide_planes.bin", "wide_tbs.bin"] and meta[n]["wide.ok"] == "1"
    for n in ("wide_beyond_limit", "largest", "wide_embed_beyond_f16"):
        assert files[n] == ["generic.bin"] and meta[n]["wide.ok"] == "0"
    assert meta["wide_unaligned"]["wide.cinP"] == "32 96 128 32 96 128"
    assert meta["wide_unaligned"]["wide.coutP"] == "96 128 64 96 128 64" and meta["wide_unaligned"]["wide.F3P"] == "64"
    assert meta["smaller"]["generic.dims"] == "5 24 40 16 8 12" and meta["smaller"]["built.cout"] == "64 64 32 64 64 32"
    assert meta["shipped"]["built.f16_ok"] == "1" and meta["shipped"]["built.head_f16"] == "1"
    assert meta["edgeconv_beyond_f16"]["built.f16_ok"] == "0"
    # (the planes of such a handle are still written: the digest of built.bin covers them)
    assert meta["edgeconv_beyond_f16"]["built.floats"] == meta["shipped"]["built.floats"]
    assert meta["head_beyond_f16"]["built.head_f16"] == "0" and meta["head_beyond_f16"]["generic.head_f16"] == "0"
    assert meta["head_beyond_f16"]["built.f16_ok"] == "1"
    assert meta["head_zero"]["built.head_scale"] == "0x1p+0" and meta["head_zero"]["built.head_f16"] == "1"
    # -0.0 can occur where a real weight is 0: the generated blobs hold exact zeros and negative gammas
    dims, blob = all_cases["smaller"]
    cout, cin2 = block_shapes(dims)[0]
    assert np.any(blob[:cout * cin2] == 0.0) and np.any(blob[cout * cin2:cout * cin2 + cout] < 0.0)

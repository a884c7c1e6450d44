"""The second public header, include/xgpr_hip_pool.h, held to what tests/test_cabi.py and tests/test_guarded_host.py hold
include/xgpr_hip.h to (their tables live inside those files and name the first header's entry points one by one): every function it
declares is exported by the built library, bound in ``_lib.POOL_SIGNATURES``, has a row in the memory-contract file of its own
(tests/test_gpu_pool_memory_contract.py), and the header is part of what ``build.py``'s ``source_id()`` hashes.  No GPU."""
import ctypes
import os
import re
import shutil

from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_pool.h")


def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_the_token_maxpool_entry_and_nothing_of_the_first_header():
    names = _declared()
    assert "xgpr_conv_token_maxpool_f32" in names
    import test_cabi
    assert not set(names) & set(test_cabi._declared())
    assert "int xgpr_conv_token_maxpool_f32(const uint8_t *tokens, const float *table, float *out," in open(HEADER).read()


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_pool.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.POOL_SIGNATURES) == set(_declared())
    assert not set(_lib.POOL_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS))
    lib = _lib.load()
    for name, args in _lib.POOL_SIGNATURES.items():                                  # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_int


def test_every_declared_entry_point_has_a_memory_contract_row():
    import test_gpu_pool_memory_contract as table
    writers = {n for n in _declared() if not n.endswith("_workspace_bytes")}
    assert len(writers) >= 1
    covered = table.covered_entry_points()
    assert covered == writers, (sorted(writers - covered), sorted(covered - writers))


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.POOL_HDR, HEADER) and bm.POOL_HDR in bm.sources()
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_pool.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "POOL_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before

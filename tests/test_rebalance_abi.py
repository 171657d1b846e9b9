"""lance_hip_reassign_rows, lance_hip_index_split and lance_hip_index_join at every layer of the boundary: declared in include/lance_hip.h, exported by the library and bound in
lance_amd/_lib.py with the declared signatures, declared in integration/rust/lance-linalg/src/hip.rs, present on the Python surface --
and the refusals that are decided before any device call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the declarations' parameter types, in order
DECLARED = {
    "lance_hip_reassign_rows": ["lance_hip_ctx *", "int", "int", "const float *", "uint64_t", "uint32_t", "const uint64_t *", "uint64_t",
                                "const uint32_t *", "const float *", "const uint32_t *", "uint32_t", "const float *", "uint32_t", "uint32_t",
                                "uint32_t *"],
    "lance_hip_index_split": ["lance_hip_ctx *", "const lance_hip_index *", "uint32_t", "const float *", "const float *", "uint64_t",
                              "lance_hip_index **"],
    "lance_hip_index_join": ["lance_hip_ctx *", "const lance_hip_index *", "uint32_t", "const float *", "uint64_t", "lance_hip_index **"],
}
CTYPE = {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "lance_hip_index **": C.POINTER(C.c_void_p)}


def library():
    import __graft_entry__ as g
    from lance_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib, _lib.load()


def test_declared_exported_and_bound():
    _lib, lib = library()
    header = open(os.path.join(ROOT, "include", "lance_hip.h")).read()
    hip_rs = open(os.path.join(ROOT, "integration", "rust", "lance-linalg", "src", "hip.rs")).read()
    for name, declared in DECLARED.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name + " is not declared"
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\b\w+$", "", p).strip() for p in params]      # drop the parameter's name
        assert types == declared, (name, types)
        fn = getattr(lib, name)
        assert name in _lib.SYMBOLS and fn.restype is C.c_int, name
        assert list(fn.argtypes) == [CTYPE.get(t, C.c_void_p) for t in declared], name
        assert re.search(r"pub fn " + name + r"\(", hip_rs), name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    assert "#define LANCE_HIP_REASSIGN_SPLIT 0" in header and "#define LANCE_HIP_REASSIGN_JOIN 1" in header
    assert (_lib.REASSIGN_SPLIT, _lib.REASSIGN_JOIN) == (0, 1)
    assert "rebalance.hip" in open(os.path.join(ROOT, "lance_amd", "csrc", "Makefile")).read()


def test_refusals_that_need_no_device():
    _lib, lib = library()
    call = lambda *a: lib.lance_hip_reassign_rows(*a)
    err = lambda: lib.lance_hip_last_error().decode()
    # a NULL context is refused before anything else is looked at
    assert call(None, 0, 0, None, 0, 8, None, 0, None, None, None, 0, None, 0, 1, None) == _lib.EINVAL and "NULL context" in err()
    h = C.c_void_p()
    assert lib.lance_hip_index_split(None, None, 0, None, None, 0, C.byref(h)) == _lib.EINVAL and "index_split: NULL argument" in err()
    assert lib.lance_hip_index_join(None, None, 0, None, 0, C.byref(h)) == _lib.EINVAL and "index_join: NULL argument" in err()
    assert h.value is None


def test_python_surface():
    pytest.importorskip("torch")
    import lance_amd
    from lance_amd import engine, vector
    assert callable(engine.Engine.reassign_rows)
    for cls in (engine.DeviceIndex, engine.DeviceFlatIndex, engine.DeviceSqIndex):
        assert all(hasattr(cls, m) for m in ("split", "join")), cls
    import inspect
    for cls in (vector.IvfPqIndex, vector.IvfFlatIndex, vector.IvfSqIndex):
        assert all(hasattr(cls, m) for m in ("split_partition", "join_partition")), cls
        sig = inspect.signature(cls.append).parameters
        assert sig["rebalance"].default is False and sig["target_partition_size"].default is None and sig["seed"].default == 0
        for m in (cls.remap, cls.delete):
            sig = inspect.signature(m).parameters
            assert sig["rebalance"].default is False and sig["target_partition_size"].default is None
    with pytest.raises(NotImplementedError, match="IVF_RQ"):
        vector.IvfRqIndex.split_partition(vector.IvfRqIndex.__new__(vector.IvfRqIndex), 0, None)
    for name in ("target_partition_size", "should_split", "should_join"):
        assert getattr(lance_amd, name) is getattr(vector, name)
    assert vector.should_split([1, 9, 9], 2) == 1 and vector.should_join([1, 0, 0], 8) == 1
    for cls in (vector.IvfPqIndex, vector.IvfFlatIndex, vector.IvfSqIndex):      # today's calls keep today's signature
        assert all(hasattr(cls, m) for m in ("append", "remap", "delete"))

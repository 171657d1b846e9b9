"""The three index-maintenance entry points at every layer of the boundary: declared in include/lance_hip.h, exported by the library
and bound in lance_amd/_lib.py, declared in integration/rust/lance-linalg/src/hip.rs, and present on the Python surface."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lance_hip_index_merge", "lance_hip_index_remap", "lance_hip_index_export_rows")


def test_declared_exported_and_bound():
    import __graft_entry__ as g
    from lance_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lance_hip.h")).read()
    hip_rs = open(os.path.join(ROOT, "integration", "rust", "lance-linalg", "src", "hip.rs")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None, name
        assert re.search(r"pub fn " + name + r"\(", hip_rs), name
    assert "#define LANCE_HIP_ROW_DELETED 0xFFFFFFFFFFFFFFFFull" in header and _lib.ROW_DELETED == 2 ** 64 - 1
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "lance_hip_index_merge" in open(os.path.join(ROOT, doc)).read(), doc


def test_python_surface():
    torch = pytest.importorskip("torch")
    import lance_amd
    from lance_amd import engine, vector
    assert callable(lance_amd.merge_indices)
    for cls in (engine.DeviceIndex, engine.DeviceFlatIndex, engine.DeviceSqIndex):
        assert all(hasattr(cls, m) for m in ("merge", "remap", "export_rows")), cls
    for cls in (vector.IvfPqIndex, vector.IvfFlatIndex, vector.IvfSqIndex):
        assert all(hasattr(cls, m) for m in ("append", "remap", "delete", "export_rows")), cls
    old, new = vector._mapping_arrays({7: None, 3: 1 << 40})
    assert sorted(zip(old.tolist(), new.tolist())) == [(3, 1 << 40), (7, 2 ** 64 - 1)]
    old, new = vector._mapping_arrays(([1, 2], [-1, None]))
    assert new.tolist() == [2 ** 64 - 1] * 2
    with pytest.raises(ValueError):
        vector._mapping_arrays(([1, 2], [3]))
    with pytest.raises(ValueError):
        lance_amd.merge_indices([])

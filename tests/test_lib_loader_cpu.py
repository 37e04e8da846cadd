"""The loader mechanism of reflector_ekf_slam_amd/_lib.py on plain Python stand-ins for a library: what a Feature and a Library
check, what their LibraryMissing says, and that ``ready`` is set by a load that succeeded and by nothing else; and the lifetime and
pending-submit rules of the handle base.  Needs no GPU and no built library."""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace as NS

import pytest

from reflector_ekf_slam_amd import _lib

HINT = "rebuild it (python __graft_entry__.py)"


class Rec(C.Structure):
    _fields_ = [("a", C.c_int), ("p", C.c_void_p), ("x", C.c_double)]        # 24 bytes


class Base:
    """A stand-in for a loaded base (a Library or a Feature): callable, counts its calls, answers with ``lib``."""

    def __init__(self, lib):
        self.lib, self.calls = lib, 0

    def __call__(self):
        self.calls += 1
        return self.lib


def good():
    return NS(f_submit=lambda: 0, f_collect=lambda: 0, f_sizeof_rec=lambda: 24)


def feature(base, declared, names=("f_submit", "f_collect")):
    return _lib.Feature(base, "libfake.so", names, [("f_sizeof_rec", Rec)], declared.append)


def test_a_missing_name_is_reported_by_name_and_several_are_all_named():
    lib = good()
    del lib.f_collect
    declared = []
    f = feature(Base(lib), declared)
    with pytest.raises(_lib.LibraryMissing) as e:
        f()
    assert "f_collect" in str(e.value) and "f_submit" not in str(e.value) and "libfake.so" in str(e.value) and HINT in str(e.value)
    assert f.ready is None and declared == []
    # the sizeof call counts among the names
    with pytest.raises(_lib.LibraryMissing) as e:
        feature(Base(NS(f_submit=lambda: 0)), declared)()
    assert "f_collect" in str(e.value) and "f_sizeof_rec" in str(e.value) and "f_submit" not in str(e.value)
    assert declared == []


def test_a_size_mismatch_reports_both_numbers():
    lib = good()
    lib.f_sizeof_rec = lambda: 16
    declared = []
    f = feature(Base(lib), declared)
    with pytest.raises(_lib.LibraryMissing) as e:
        f()
    assert "16" in str(e.value) and "24" in str(e.value) and "libfake.so" in str(e.value) and HINT in str(e.value)
    assert f.ready is None and declared == []


def test_after_a_failure_a_good_base_succeeds_and_the_result_is_cached():
    bad, lib = good(), good()
    del bad.f_submit
    base, declared = Base(bad), []
    f = feature(base, declared)
    with pytest.raises(_lib.LibraryMissing):
        f()
    bad.f_submit, bad.f_sizeof_rec = (lambda: 0), (lambda: 32)
    with pytest.raises(_lib.LibraryMissing):
        f()
    assert f.ready is None and base.calls == 2
    base.lib = lib
    assert f() is lib and f.ready is lib and declared == [lib]
    # a second call touches neither the base nor declare
    assert f() is lib and base.calls == 3 and declared == [lib]


def test_a_feature_on_a_feature_resolves_through_it():
    lib, declared = good(), []
    base = Base(lib)
    first = feature(base, declared, names=("f_submit",))
    second = _lib.Feature(first, "libfake.so", ("f_collect",), (), declared.append)
    assert first.ready is None and second.ready is None
    assert second() is lib and first.ready is lib and second.ready is lib and declared == [lib, lib] and base.calls == 1
    assert second() is lib and first() is lib and base.calls == 1 and declared == [lib, lib]
    # the first one's calls keep working when the second one's are absent
    del lib.f_collect
    first.ready = second.ready = None
    with pytest.raises(_lib.LibraryMissing) as e:
        second()
    assert "f_collect" in str(e.value) and first.ready is lib and second.ready is None


def test_a_root_loader_names_the_path_it_did_not_find(monkeypatch, tmp_path):
    declared = []
    root = _lib.Library("libnone.so", ("none_abi_version", 1), declared.append)
    monkeypatch.setattr(_lib, "lib_path", lambda name: os.path.join(str(tmp_path), "no_such_dir", name))      # (looked up at call time)
    with pytest.raises(_lib.LibraryMissing) as e:
        root()
    assert os.path.join(str(tmp_path), "no_such_dir", "libnone.so") in str(e.value) and HINT in str(e.value)
    assert root.ready is None and declared == []
    root.ready = lib = good()                                     # what a successful load leaves: returned as it is
    assert root() is lib and declared == []


def test_the_handle_base_frees_once_and_keeps_the_one_pending_submit():
    freed = []

    class H(_lib.Handle):
        _destroy = "h_destroy"

        def _error(self, rc, where):
            return RuntimeError(f"{where}: {rc}")

    bare = object.__new__(H)                                      # never initialised: nothing to free, nothing raised
    bare.close()
    assert freed == [] and bare._pending is None
    h = H()
    h._L, h._h = NS(h_destroy=freed.append), 7
    assert h._submitted(-1, "a") == -1 and h._pending is None     # a refused submit is not pending
    assert h._submitted(0, "a") == 0 and h._pending == "a"
    assert h._collected(-5) == -5 and h._pending == "a"           # a refused collect leaves it pending
    assert h._collected(0) == 0 and h._pending is None
    h._chk(0, "call")
    with pytest.raises(RuntimeError, match="call: -3"):
        h._chk(-3, "call")
    with pytest.raises(RuntimeError, match="call.*-3"):            # a class that names no exception of its own
        _lib.Handle()._chk(-3, "call")
    h.close()
    h.close()
    del h
    assert freed == [7]

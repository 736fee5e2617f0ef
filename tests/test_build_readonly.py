"""Up-to-date libraries are returned without the build lock: a user who
cannot write the tree (another user built it) still loads them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_up_to_date_libraries_need_no_lock_and_no_write(monkeypatch):
    from pbs_amd import build
    core, hip = build.build_all()  # a no-op after the in-tree build
    before = {p: os.stat(p).st_mtime_ns for p in (core, hip, core + ".stamp", hip + ".stamp")}

    def denied(self):
        raise PermissionError(13, "Permission denied", os.path.join(build.LIBDIR, ".build.lock"))

    monkeypatch.setattr(build._BuildLock, "__enter__", denied)
    assert build.build_core() == core
    assert build.build_hip() == hip
    assert build.build_all() == (core, hip)
    assert before == {p: os.stat(p).st_mtime_ns for p in before}

"""MIOpen's user find-db for the tests, ``bench.py`` and the tools: a working copy of tools/miopen_db.

tools/miopen_db ships the find results of the regulariser's convolutions, so a fresh box skips most of
the multi-minute search.  MIOpen rewrites the files under MIOPEN_USER_DB_PATH whenever it runs, so
pointing it at the tracked files modifies them on every GPU run (and needs a writable checkout).
``use()`` copies them into a temporary directory of this process, removed when it exits, and points
MIOpen there; child processes inherit the path.  Must run before torch initialises MIOpen.  A
MIOPEN_USER_DB_PATH already set is left alone.
"""
import atexit
import os
import shutil
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHIPPED = os.path.join(REPO, "tools", "miopen_db")


def _remove(path, owner):
    if os.getpid() == owner:   # not from a forked child that runs the parent's exit handlers
        shutil.rmtree(path, ignore_errors=True)


def use():
    if "MIOPEN_USER_DB_PATH" in os.environ:
        return os.environ["MIOPEN_USER_DB_PATH"]
    work = tempfile.mkdtemp(prefix="mvs_miopen_db_")
    atexit.register(_remove, work, os.getpid())
    for name in os.listdir(SHIPPED):
        if not name.startswith("."):
            shutil.copyfile(os.path.join(SHIPPED, name), os.path.join(work, name))
    os.environ["MIOPEN_USER_DB_PATH"] = work
    return work

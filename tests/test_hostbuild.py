"""tests/hostsim/hostbuild.py: the table names every host source once, and a product is rebuilt exactly when the command line
or the bytes of a file that g++ reported change -- not when a file time does, not when the tree moves -- and never replaced
by a failed compile.  The staleness rules run on a two-file tree in tmp_path through hostbuild.build, the function under
load() and build_all(); the last test reads what g++ recorded for the project's own libraries."""
import ctypes
import glob
import os
import shutil

import pytest

from hostsim import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = hostbuild.SHARED + hostbuild.STRICT
NAME = "libanswer.so"
CSRC = "vanishing_points_2017_amd/csrc/"


def test_the_table_names_every_source_once():
    sims = sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "hostsim", "sim_*.cpp"))) + ["pm_driver.cpp"]
    assert sorted(src for src, _ in hostbuild.LIBS.values()) == sorted(sims)
    drivers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "hostsim", "*_driver.cpp")))
    drivers.remove("pm_driver.cpp")
    assert sorted(src for src, _ in hostbuild.DRIVERS.values()) == drivers
    for src, _ in list(hostbuild.LIBS.values()) + list(hostbuild.DRIVERS.values()):
        assert os.path.exists(os.path.join(HERE, "hostsim", src)), src
    names = [hostbuild.lib_name(k) for k in hostbuild.LIBS]
    assert len(set(names)) == len(names) == 24


def _tree(root, value=41):
    """<root>/src/answer.cpp including <root>/inc/answer.hpp; products go to <root>/out"""
    os.makedirs(os.path.join(root, "src"))
    os.makedirs(os.path.join(root, "inc"))
    with open(os.path.join(root, "src", "answer.cpp"), "w") as f:
        f.write('#include "../inc/answer.hpp"\nextern "C" int answer() { return ANSWER; }\n')
    _header(root, value)


def _header(root, value):
    with open(os.path.join(root, "inc", "answer.hpp"), "w") as f:
        f.write("#define ANSWER %s\n" % value)


def _build(root, flags=FLAGS):
    return hostbuild.build(os.path.join(root, "src", "answer.cpp"), flags, os.path.join(root, "out"), NAME, root=root)


def _state(root):
    """name -> bytes of everything in the output directory"""
    out = os.path.join(root, "out")
    state = {}
    for name in sorted(os.listdir(out)):
        with open(os.path.join(out, name), "rb") as f:
            state[name] = f.read()
    return state


def _compiled(root, flags=FLAGS):
    """whether a call of build() compiled: it then renames a new file over the library, so the path names another inode
    (the contents cannot tell: the same inputs give the same library and the same stamp)"""
    so = os.path.join(root, "out", NAME)
    before = os.stat(so).st_ino
    _build(root, flags)
    return os.stat(so).st_ino != before


def _answer(root):
    # dlopen caches by path, and the library at this path changes: load a copy under a name of its own
    copy = os.path.join(root, "loaded_%d.so" % len(os.listdir(root)))
    shutil.copy(os.path.join(root, "out", NAME), copy)
    return ctypes.CDLL(copy).answer()


def test_staleness_follows_bytes_and_flags_not_file_times(tmp_path):
    root = str(tmp_path)
    _tree(root)
    so = _build(root)
    assert so == os.path.join(root, "out", NAME) and sorted(os.listdir(os.path.dirname(so))) == [NAME, NAME + ".d", NAME + ".stamp"]
    assert _answer(root) == 41
    with open(so + ".stamp") as f:
        stamp = f.read()
    assert not _compiled(root)                                           # a second call
    header = os.path.join(root, "inc", "answer.hpp")
    os.utime(header, (os.path.getatime(header), os.stat(so).st_mtime + 3600))
    os.utime(os.path.join(root, "src", "answer.cpp"), None)
    assert not _compiled(root)                                           # newer file times alone
    _header(root, 42)
    assert _compiled(root) and _answer(root) == 42                       # one byte of the header
    with open(so + ".stamp") as f:
        assert f.read() != stamp
    assert not _compiled(root)
    assert _compiled(root, FLAGS + ["-DUNUSED=1"])                       # the flags
    assert not _compiled(root, FLAGS + ["-DUNUSED=1"])
    os.remove(so + ".d")
    assert _compiled(root, FLAGS + ["-DUNUSED=1"]) and os.path.exists(so + ".d")    # no dependency file
    os.remove(so + ".stamp")
    assert _compiled(root, FLAGS + ["-DUNUSED=1"])                       # no stamp
    os.rename(header, header + ".away")
    with pytest.raises(RuntimeError):                                    # a listed dependency is missing: stale, and g++ says so
        _build(root, FLAGS + ["-DUNUSED=1"])


def test_a_failed_compile_leaves_the_previous_product(tmp_path, capfd):
    root = str(tmp_path)
    _tree(root)
    _build(root)
    before = _state(root)
    assert sorted(before) == [NAME, NAME + ".d", NAME + ".stamp"]
    _header(root, "41 +")
    with pytest.raises(RuntimeError, match="answer.cpp"):
        _build(root)
    assert "error" in capfd.readouterr().err
    assert _state(root) == before                                        # the three files byte for byte, and no fourth
    _header(root, 43)
    assert _compiled(root) and _answer(root) == 43


def test_a_copied_tree_is_fresh(tmp_path):
    first, second = str(tmp_path / "first"), str(tmp_path / "elsewhere" / "second")
    os.makedirs(first)
    _tree(first)
    _build(first)
    shutil.copytree(first, second)
    before = _state(second)
    assert before == _state(first)
    assert not _compiled(second) and _state(second) == before
    _header(second, 44)
    assert _compiled(second) and not _compiled(first)


def test_the_recorded_dependencies_are_the_compilers():
    for key in ("prior", "lines", "overlay", "estep", "em_plan", "raster"):   # the six whose hand-kept lists lacked it
        hostbuild.load(key)
        assert CSRC + "wave_prims.hpp" in hostbuild.recorded_deps(key), key
    hostbuild.load("cnn_model")
    assert hostbuild.recorded_deps("cnn_model") == ["tests/hostsim/sim_cnn_model.cpp", CSRC + "cnn_model.hpp"]
    hostbuild.load("em")
    em = hostbuild.recorded_deps("em")
    assert "tests/hostsim/sim_em.cpp" in em and CSRC + "em_device.hpp" in em
    assert not [d for d in em if os.path.basename(d).startswith("cnn_")]

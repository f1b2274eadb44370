"""The three-source build (opticalflow_amd/build.py): every kernel header belongs to exactly one source,
the staleness rule follows the depfiles, and the library exports the C ABI of include/vof.h and nothing of vof::host.
Reads source and the library the session fixture built; compiles nothing."""
import os
import re
import subprocess
import time

from conftest import ROOT
from opticalflow_amd import build

HOST_PREFIX = "_ZN3vof4host"          # what every name of namespace vof::host (csrc/vof_host.hpp) is mangled to start with


def includes(name, seen=None):
    """Every file of csrc/ that `name` reaches through #include "..." lines, itself included."""
    seen = set() if seen is None else seen
    if name in seen:
        return seen
    seen.add(name)
    with open(os.path.join(build.CSRC, name)) as f:
        for inc in re.findall(r'^\s*#include "([^"]+)"', f.read(), flags=re.M):
            if os.path.exists(os.path.join(build.CSRC, inc)) and os.sep not in inc:
                includes(inc, seen)
    return seen


def test_every_kernel_header_belongs_to_one_source():
    assert build.SOURCES == ["vof.hip", "vof_pairs.hip", "vof_frames.hip"]
    reach = {src: includes(src) for src in build.SOURCES}
    headers = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hpp"))
    assert "vof_host.hpp" in headers and "vof_shared.hpp" in headers
    for h in headers:
        owners = [src for src in build.SOURCES if h in reach[src]]
        assert owners, h + " is reached from no source"
        with open(os.path.join(build.CSRC, h)) as f:
            if "__global__" in re.sub(r"//[^\n]*", "", f.read()):
                assert len(owners) == 1, "%s defines kernels and is reached from %s" % (h, owners)
    for shared in ("vof_host.hpp", "vof_shared.hpp"):
        assert all(shared in reach[src] for src in build.SOURCES)


def fake_tree(tmp_path):
    """csrc/ with three sources and four headers, include/vof.h two levels up as in the repository, objects and hand-written
    depfiles: a.hip -> one.hpp, shared.hpp; b.hip -> two.hpp, shared.hpp, the public header; c.hip has no depfile."""
    csrc = tmp_path / "pkg" / "csrc"
    objdir = csrc / "_obj"
    objdir.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    old = time.time() - 1000
    for p in [csrc / n for n in ("a.hip", "b.hip", "c.hip", "one.hpp", "two.hpp", "shared.hpp", "lonely.hpp")] + [tmp_path / "include" / "vof.h"]:
        p.write_text("// " + p.name + "\n")
        os.utime(p, (old, old))
    for n in ("a", "b", "c"):
        (objdir / (n + ".o")).write_text("")
        os.utime(objdir / (n + ".o"), (old + 100, old + 100))
    (objdir / "a.d").write_text("_obj/a.o: a.hip \\\n  one.hpp shared.hpp\n")
    (objdir / "b.d").write_text("_obj/b.o: b.hip two.hpp \\\n  shared.hpp ../../include/vof.h\n")
    return str(csrc), str(objdir), ["a.hip", "b.hip", "c.hip"]


def touch(csrc, name):
    now = time.time()
    os.utime(os.path.join(csrc, name), (now, now))


def test_staleness_follows_the_depfiles(tmp_path):
    csrc, objdir, sources = fake_tree(tmp_path)
    assert build.stale_sources(csrc, objdir, sources) == []                                   # nothing touched: nothing stale
    assert build.default_deps(csrc, "c.hip") == ["c.hip", "lonely.hpp", "one.hpp", "shared.hpp", "two.hpp", build.PUBLIC_HEADER]
    touch(csrc, "one.hpp")
    assert build.stale_sources(csrc, objdir, sources) == ["a.hip", "c.hip"]                   # c.hip has no depfile: any header
    csrc, objdir, sources = fake_tree(tmp_path / "second")
    touch(csrc, "shared.hpp")
    assert build.stale_sources(csrc, objdir, sources) == ["a.hip", "b.hip", "c.hip"]
    csrc, objdir, sources = fake_tree(tmp_path / "third")
    touch(csrc, "lonely.hpp")                                                                 # no depfile names it
    assert build.stale_sources(csrc, objdir, sources) == ["c.hip"]
    csrc, objdir, sources = fake_tree(tmp_path / "fourth")
    touch(csrc, build.PUBLIC_HEADER)
    assert build.stale_sources(csrc, objdir, sources) == ["b.hip", "c.hip"]
    touch(csrc, "a.hip")
    assert build.stale_sources(csrc, objdir, sources) == ["a.hip", "b.hip", "c.hip"]
    csrc, objdir, sources = fake_tree(tmp_path / "fifth")
    os.remove(os.path.join(objdir, "b.o"))                                                    # a missing object is stale ...
    assert build.stale_sources(csrc, objdir, sources) == ["b.hip"]
    lib = os.path.join(csrc, "lib.so")
    open(lib, "w").close()                                                                    # ... unless the library is there without it
    assert build.stale_sources(csrc, objdir, sources, lib=lib) == []
    touch(csrc, "two.hpp")
    assert build.stale_sources(csrc, objdir, sources, lib=lib) == ["b.hip", "c.hip"]
    os.remove(os.path.join(csrc, "one.hpp"))                                                  # a named file that is gone
    assert build.stale_sources(csrc, objdir, sources, lib=lib) == ["a.hip", "b.hip", "c.hip"]


def test_a_non_default_build_keeps_its_objects_to_itself(tmp_path):
    assert build.object_dir() == os.path.join(build.CSRC, "_obj") == build.object_dir(build.LIB)
    other = build.object_dir(str(tmp_path / "libvof_b.so"))
    assert other == str(tmp_path / "libvof_b_obj") and other != build.object_dir()


def test_the_library_exports_the_c_abi_and_nothing_of_the_internal_namespace():
    readelf = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "llvm", "bin", "llvm-readelf")
    out = subprocess.run([readelf, "--dyn-syms", "-W", build.LIB], check=True, capture_output=True, text=True).stdout
    defined = [f[7] for f in (line.split() for line in out.splitlines()) if len(f) == 8 and f[0].rstrip(":").isdigit() and f[6] != "UND"]
    with open(os.path.join(ROOT, "include", "vof.h")) as f:
        header = re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(vof_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 80
    assert sorted(s for s in defined if s.startswith("vof_")) == sorted(declared)
    assert not [s for s in defined if HOST_PREFIX in s]
    with open(os.path.join(build.CSRC, "vof_host.hpp")) as f:
        assert re.search(r'namespace vof \{\s*namespace host __attribute__\(\(visibility\("hidden"\)\)\) \{', f.read())

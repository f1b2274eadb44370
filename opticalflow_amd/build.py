"""Build the native library (libvof.so) in-tree with hipcc for gfx950: one object per source, compiled side by side, one link."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libvof.so")
SOURCES = ["vof.hip", "vof_pairs.hip", "vof_frames.hip"]
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-fPIC", "-pthread"]
PUBLIC_HEADER = os.path.join("..", "..", "include", "vof.h")   # from csrc/, where the compiler runs


def object_dir(output=LIB):
    """Where the objects and depfiles of the library at `output` live: csrc/_obj, or a directory named after a non-default output."""
    if os.path.abspath(output) == LIB:
        return os.path.join(CSRC, "_obj")
    return os.path.splitext(os.path.abspath(output))[0] + "_obj"


def default_deps(csrc, source):
    """What a source without a depfile is taken to depend on: itself, every header of csrc/ and the public header."""
    deps = [source] + sorted(f for f in os.listdir(csrc) if f.endswith((".hpp", ".h")))
    return deps + ([PUBLIC_HEADER] if os.path.exists(os.path.join(csrc, PUBLIC_HEADER)) else [])


def depfile_deps(path):
    """The prerequisites a compiler-written depfile (-MMD) names, or None where there is none."""
    if not os.path.exists(path):
        return None
    with open(path) as f:
        text = f.read().replace("\\\n", " ")
    return text.split(":", 1)[1].split() if ":" in text else None


def stale_sources(csrc, objdir, sources=SOURCES, lib=None):
    """The sources to compile again: the object is missing, or older than a file its depfile names (paths relative to csrc/; a
    named file that is gone counts as newer).  Without a depfile default_deps stands in.  Where the library `lib` travelled
    without its objects, its own time stands in for a missing object's: a library newer than everything it was built from is
    not built again."""
    stale = []
    for src in sources:
        stem = os.path.splitext(src)[0]
        obj = os.path.join(objdir, stem + ".o")
        made = obj if os.path.exists(obj) else lib
        if not made or not os.path.exists(made):
            stale.append(src)
            continue
        t = os.path.getmtime(made)
        deps = depfile_deps(os.path.join(objdir, stem + ".d")) or default_deps(csrc, src)
        paths = [os.path.join(csrc, d) for d in deps]
        if any(not os.path.exists(p) or os.path.getmtime(p) > t for p in paths):
            stale.append(src)
    return stale


def objects(objdir, sources=SOURCES):
    return [os.path.join(objdir, os.path.splitext(s)[0] + ".o") for s in sources]


def needs_link(lib, objdir, sources=SOURCES):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.exists(o) and os.path.getmtime(o) > t for o in objects(objdir, sources))


def needs_build():
    objdir = object_dir()
    return bool(stale_sources(CSRC, objdir, lib=LIB)) or needs_link(LIB, objdir)


def build_native(force=False, verbose=True, output=None, extra_flags=()):
    """Compile every HIP source for gfx950 into opticalflow_amd/csrc/libvof.so, or into `output` with `extra_flags` added (an A/B
    build: its objects live next to it and the default build is left alone)."""
    lib = os.path.abspath(output) if output else LIB
    objdir = object_dir(lib)
    todo = list(SOURCES) if force else stale_sources(CSRC, objdir, lib=lib)
    if not todo and not needs_link(lib, objdir):
        return lib
    todo += [s for s, o in zip(SOURCES, objects(objdir)) if s not in todo and not os.path.exists(o)]   # the link needs them all
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(objdir, exist_ok=True)
    running = []
    for src in todo:                                   # one compiler process per source, all at once
        stem = os.path.join(objdir, os.path.splitext(src)[0])
        cmd = [hipcc] + FLAGS + list(extra_flags) + ["-c", "-MMD", "-MF", stem + ".d", "-o", stem + ".o", src]
        if verbose:
            print("[opticalflow_amd] " + " ".join(cmd), file=sys.stderr)
        running.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
    failed = [(cmd, p.returncode) for cmd, p in running if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(failed[0][1], failed[0][0])
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", lib] + objects(objdir)
    if verbose:
        print("[opticalflow_amd] " + " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, cwd=CSRC, check=True)
    return lib


if __name__ == "__main__":
    # python -m opticalflow_amd.build [--force] [--output PATH] [-- extra compiler flags]
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    out = argv[argv.index("--output") + 1] if "--output" in argv else None
    build_native(force="--force" in argv, output=out, extra_flags=extra)

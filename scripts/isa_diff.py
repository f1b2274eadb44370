#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the library, instruction for instruction (no GPU needed).
usage: isa_diff.py [-v] OLD.so NEW.so [substring ...]     (substrings select kernels by their demangled name)

The code objects are extracted with `llvm-objdump --offloading`, the kernels are listed from the amdhsa.kernels note, and for each
kernel the note entry (register counts, scratch, LDS, kernel arguments) and the disassembly are compared as text.  Two things that
depend on where a function lies and not on what it does are normalised: the s_nop padding behind its last instruction, and the
literal of the instruction that follows an s_getpc_b64 (a pc-relative address).  Prints the kernel counts, the symbols only one
side has, and how many note entries and functions differ; -v adds a unified diff per differing kernel."""
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile


def llvm_bin():
    """The ROCm tree's lib/llvm/bin, found from where hipcc lies."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for d in (os.path.join(root, "lib", "llvm", "bin"), os.path.join(root, "llvm", "bin")):
        if os.path.exists(os.path.join(d, "llvm-objdump")):
            return d
    sys.exit("isa_diff: no llvm-objdump under " + root)


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_objects(lib, tmp):
    """Extract the gfx950 code objects of `lib` into a directory of their own under tmp."""
    d = tempfile.mkdtemp(dir=tmp)
    name = os.path.join(d, "lib.so")
    shutil.copy(lib, name)
    run("llvm-objdump", "--offloading", name, cwd=d)
    return sorted(f for f in glob.glob(name + ".*") if "gfx950" in f)


def note_entries(co):
    """kernel symbol -> its entry of the amdhsa.kernels note, as text."""
    txt = run("llvm-readelf", "--notes", co)
    m = re.search(r"^amdhsa\.kernels:\n(.*?)(?=^\S)", txt, re.M | re.S)
    entries = {}
    for e in re.split(r"^  - ", m.group(1) if m else "", flags=re.M)[1:]:
        sym = re.search(r"^\s*\.symbol:\s*(\S+)", e, re.M).group(1)
        entries[sym[:-3] if sym.endswith(".kd") else sym] = e.rstrip() + "\n"
    return entries


def functions(co):
    """symbol -> normalised disassembly lines of every function of the code object."""
    out, name, after_getpc = {}, None, False
    for line in run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        ins = line.split("//")[0].strip()
        if name is None or not ins:
            continue
        if after_getpc:
            ins = re.sub(r"(0x[0-9a-f]+|-?\d+)\s*$", "PCREL", ins)
        after_getpc = ins.startswith("s_getpc_b64")
        out[name].append(ins)
    for body in out.values():
        while body and (body[-1].startswith("s_nop") or body[-1] == "..."):   # ("...": the disassembler's mark for zero fill)
            body.pop()
    return out


def load(lib, tmp):
    notes, funcs = {}, {}
    for co in code_objects(lib, tmp):
        notes.update(note_entries(co))
        funcs.update(functions(co))
    return notes, funcs


def main(argv):
    verbose = "-v" in argv
    argv = [a for a in argv if a != "-v"]
    if len(argv) < 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        (on, of), (nn, nf) = load(argv[0], tmp), load(argv[1], tmp)
    syms = sorted(set(on) | set(nn))
    pretty = dict(zip(syms, subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")))
    if argv[2:]:
        syms = [s for s in syms if any(f in pretty[s] for f in argv[2:])]
    old, new = [s for s in syms if s in on], [s for s in syms if s in nn]
    print("kernels: %d old, %d new" % (len(old), len(new)))
    for s in old:
        if s not in nn:
            print("missing in new:", pretty[s])
    for s in new:
        if s not in on:
            print("extra in new:  ", pretty[s])
    both = [s for s in old if s in nn]
    dn = [s for s in both if on[s] != nn[s]]
    df = [s for s in both if of.get(s) != nf.get(s)]
    print("note entries that differ: %d of %d" % (len(dn), len(both)))
    print("functions that differ:    %d of %d" % (len(df), len(both)))
    for s in sorted(set(dn) | set(df)):
        print("differs (%s): %s" % (" + ".join(w for w, l in (("note", dn), ("code", df)) if s in l), pretty[s]))
        if verbose:
            for a, b in ((on[s].splitlines(), nn[s].splitlines()), (of.get(s, []), nf.get(s, []))):
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a, b, "old", "new", lineterm="", n=2))
    return 1 if dn or df or len(old) != len(new) else 0


LLVM = llvm_bin()
if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

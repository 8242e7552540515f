"""One-off check for the change that made the ctypes bindings read include/*.h: the derived bindings are the hand-written
ones of the parent commit.

    git worktree add /tmp/parent HEAD~1          # a checkout of the parent commit
    python scripts/binding_identity.py /tmp/parent [--startup 20]

Compares, for _lib / _jpeglib / _jpegdeclib: every SIGNATURES entry (key order included) with `==` on the ctypes objects,
ctypes.sizeof and every field's (name, offset, size, type) of the four structs, and every public integer constant of the
parent's modules.  POINTER(struct) cannot be `==` across two class objects of the same struct: such an entry is compared as
("POINTER", the struct's layout).  --startup N times `from text2video_amd import _lib; _lib.load()` in N fresh processes per
tree, interleaved, both on this tree's libt2v_hip.so (T2V_LIBRARY).  Exit status 1 on any difference.
"""
import argparse
import ctypes
import importlib.util
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("_lib", "_jpeglib", "_jpegdeclib")
STRUCTS = ("ConvDesc", "GenDesc", "Layer", "GenIO")


def layout(s):
    return (ctypes.sizeof(s), tuple((n, getattr(s, n).offset, getattr(s, n).size, t) for n, t in s._fields_))


def norm(t):
    if isinstance(t, type) and issubclass(t, ctypes._Pointer) and issubclass(t._type_, ctypes.Structure):
        return ("POINTER", layout(t._type_))
    return t


def parent_module(tree, name):
    spec = importlib.util.spec_from_file_location("parent" + name, os.path.join(tree, "text2video_amd", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)        # (the parent's modules import nothing of their package until load())
    return mod


def startup(tree, runs):
    env = dict(os.environ, T2V_LIBRARY=os.path.join(ROOT, "text2video_amd", "lib", "libt2v_hip.so"))
    times = {"parent": [], "head": []}
    for _ in range(runs):
        for label, root in (("parent", tree), ("head", ROOT)):
            t0 = time.perf_counter()
            subprocess.run([sys.executable, "-c", "from text2video_amd import _lib; _lib.load()"], check=True, cwd=root,
                           env=dict(env, PYTHONPATH=root))
            times[label].append(time.perf_counter() - t0)
    for label, t in times.items():
        print("startup %-6s  runs %d  median %.1f ms  min %.1f ms  max %.1f ms"
              % (label, runs, 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)))
    over = statistics.median(times["head"]) - statistics.median(times["parent"])
    spread = max(times["parent"]) - min(times["parent"])
    print("startup head median - parent median = %+.1f ms; the parent's own spread (max - min) = %.1f ms: %s"
          % (1e3 * over, 1e3 * spread, "within" if over <= spread else "EXCEEDS"))
    return over <= spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_tree")
    ap.add_argument("--startup", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    bad = 0
    for name in MODULES:
        old, new = parent_module(args.parent_tree, name), importlib.import_module("text2video_amd." + name)
        order = list(old.SIGNATURES) == list(new.SIGNATURES)
        differ = [k for k in old.SIGNATURES if k not in new.SIGNATURES or
                  (old.SIGNATURES[k][0], [norm(a) for a in old.SIGNATURES[k][1]]) !=
                  (new.SIGNATURES[k][0], [norm(a) for a in new.SIGNATURES[k][1]])]
        print("%-12s SIGNATURES: %d entries at the parent, %d at head; entries that differ: %s; key order %s"
              % (name, len(old.SIGNATURES), len(new.SIGNATURES), differ or "none", "equal" if order else "differs:"))
        if not order:       # reported, not counted: the order only decides in which order load() sets argtypes
            header = open(os.path.join(ROOT, "include", new._binding.header.name)).read()
            at = {k: re.search(r"^[a-z_ ]+\*? %s\(" % k, header, re.M).start() for k in new.SIGNATURES}     # its prototype
            early = [k for i, k in enumerate(old.SIGNATURES) if any(at[j] < at[k] for j in list(old.SIGNATURES)[i + 1:])]
            print("%14s head has the header's order: %s; the parent's hand-written table did not: it listed %d symbols before "
                  "one the header declares earlier (%s, ...)" % ("", sorted(at, key=at.get) == list(new.SIGNATURES), len(early),
                                                                ", ".join(early[:3])))
            order = sorted(at, key=at.get) == list(new.SIGNATURES) and sorted(old.SIGNATURES) == sorted(new.SIGNATURES)
        consts = {k: v for k, v in vars(old).items() if not k.startswith("_") and type(v) is int}
        wrong = {k: (v, getattr(new, k, None)) for k, v in consts.items() if getattr(new, k, None) != v}
        print("%-12s constants: %d public integers at the parent (%s); that differ at head: %s"
              % (name, len(consts), " ".join("%s=%d" % kv for kv in consts.items()), wrong or "none"))
        bad += (not order) + len(differ) + len(wrong)
    old, new = parent_module(args.parent_tree, "_lib"), importlib.import_module("text2video_amd._lib")
    for s in STRUCTS:
        a, b = layout(getattr(old, s)), layout(getattr(new, s))
        print("%-12s sizeof %d / %d, %d fields (name, offset, size, type): %s"
              % (s, a[0], b[0], len(a[1]), "equal" if a == b else "DIFFER: %s != %s" % (a, b)))
        bad += a != b
    print("identity: %s" % ("every entry, layout and constant equal" if not bad else "%d DIFFERENCES" % bad))
    if args.startup and not startup(args.parent_tree, args.startup):
        bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

"""The C boundary, read from the headers: prototypes, structs and integer constants of include/*.h, their ctypes form, and
the one loader of the shared libraries.  Standard library only (the torch-free frame loop of vid2vid/test.py loads it).

The reader knows a closed vocabulary and raises HeaderError, naming the header and the declaration, on anything else:
  declarations   prototypes, `typedef struct { ... } name;`, `typedef struct name name;` (opaque), `enum { ... };` /
                 `typedef enum { ... } name;`, `#define NAME <integer>`; include guards, #include and extern "C";
                 `#include "x.h"` only in a companion header read with base = the Header of x.h, whose types it then uses
  scalars        int, long, float, double, size_t (and void as a return type)
  pointers       `const char*` returned -> c_char_p; a pointer to a struct of the header -> POINTER(that struct);
                 `int*` -> POINTER(c_int); `T**` (a pointer the callee writes a pointer through) -> POINTER(c_void_p);
                 every other pointer, `T* const*` (an array of pointers the callee reads) included -> c_void_p
There is no default: a type outside this list is an error, never a silent c_void_p.
"""
import ctypes
import os
import re
import threading
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
_SCALARS = {"int": c_int, "long": c_long, "float": c_float, "double": c_double, "size_t": c_size_t}
_POINTEES = {"void", "char"} | {"%sint%d_t" % (u, n) for u in ("", "u") for n in (8, 16, 32, 64)}    # behind a `*` only
_DIRECTIVE = re.compile(r'#\s*(ifndef\s+\w+|ifdef\s+__cplusplus|include\s*<\w+\.h>|endif)')
_INTEGER = re.compile(r"-?(0[xX][0-9a-fA-F]+|[1-9]\d*|0)")
_DECLARATOR = re.compile(r"(.+?)\b(\w+)((?: ?, ?\w+)*)")      # type, name, further names (`int H, W`)


class HeaderError(ValueError):
    pass


class Header:
    """functions: name -> (return type, [parameter types]) as C spells them, names removed; parameters: name -> [parameter
    names], in the same order; signatures: name -> (restype, argtypes); fields: struct name -> [(type, field)]; structs:
    struct name -> ctypes.Structure; constants: name -> int.  All in the header's order."""

    def __init__(self, text, name, base=None):
        self.name, self.base = name, base
        self.functions, self.signatures, self.fields, self.structs, self.constants, self.opaque = {}, {}, {}, {}, {}, set()
        self.parameters = {}
        text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
        code = []
        for line in text.split("\n"):
            s = line.strip()
            if not s.startswith("#"):
                code.append(line)
                continue
            m = re.fullmatch(r"#\s*define\s+(\w+)\s*(.*)", s)
            if m and m.group(2):        # (without a value: an include guard)
                self.constants[m.group(1)] = self._integer(m.group(2), s)
            elif base is not None and re.fullmatch(r'#\s*include\s*"%s"' % re.escape(base.name), s):
                continue
            elif not (m or _DIRECTIVE.fullmatch(s)):
                self._bad("a preprocessor line outside the vocabulary", s)
        text = "\n".join(code).rstrip()
        m = re.search(r'extern\s+"C"\s*\{', text)
        if m:
            if not text.endswith("}"):
                self._bad('extern "C" does not close at the end of the header', text[-60:])
            text = text[:m.start()] + text[m.end():-1]
        depth = start = 0
        for m in re.finditer(r"[{};]", text):
            depth += {"{": 1, "}": -1, ";": 0}[m.group()]
            if m.group() == ";" and depth == 0:
                decl, start = " ".join(text[start:m.start()].split()), m.end()
                if decl:
                    self._declare(decl)
        if text[start:].strip():
            self._bad("a declaration without its closing `;`", text[start:])

    def _bad(self, why, decl):
        raise HeaderError("%s: %s: `%s`" % (self.name, why, " ".join(decl.split())))

    def _integer(self, s, decl):
        if not _INTEGER.fullmatch(s):
            self._bad("`%s` is not an integer constant" % s, decl)
        return int(s, 0)

    def _declare(self, decl):
        m = re.fullmatch(r"typedef struct (\w+) (\w+)", decl)
        if m and m.group(1) == m.group(2):
            self.opaque.add(m.group(1))
            return
        m = re.fullmatch(r"typedef struct ?\{(.*)\} ?(\w+)", decl)
        if m:
            fields = []
            for f in filter(None, (f.strip() for f in m.group(1).split(";"))):
                d = _DECLARATOR.fullmatch(f)
                if not d or (d.group(3) and "*" in d.group(1)):
                    self._bad("a field outside the vocabulary (`type name[, name]`; no array, bit field or nested body)", f)
                fields += [(self._spell(d.group(1)), n) for n in [d.group(2)] + re.findall(r"\w+", d.group(3))]
            self.fields[m.group(2)] = fields
            self.structs[m.group(2)] = type(m.group(2), (ctypes.Structure,),
                                            {"_fields_": [(n, self.ctype(t, decl)) for t, n in fields],
                                             "__doc__": "%s (include/%s)." % (m.group(2), self.name)})
            return
        m = re.fullmatch(r"(?:typedef )?enum(?: \w+)? ?\{(.*)\}(?: ?\w+)?", decl)
        if m:
            value = 0
            for e in filter(None, (e.strip() for e in m.group(1).split(","))):
                d = re.fullmatch(r"(\w+)(?: ?= ?(.+))?", e)
                if not d:
                    self._bad("an enumerator outside the vocabulary", e)
                value = self._integer(d.group(2), decl) if d.group(2) else value
                self.constants[d.group(1)] = value
                value += 1
            return
        m = re.fullmatch(r"(.+?)\b(\w+) ?\(([^()]*)\)", decl)
        if not m:
            self._bad("neither a prototype (no function-pointer parameter), a struct, an enum nor an opaque typedef", decl)
        params, names = [], []
        for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            d = _DECLARATOR.fullmatch(p.strip())
            if not d or d.group(3):
                self._bad("parameter `%s`: not `type name` (variadic, nameless or empty; no parameters is `(void)`)" % p.strip(), decl)
            params.append(self._spell(d.group(1)))
            names.append(d.group(2))
        ret = self._spell(m.group(1))
        self.functions[m.group(2)] = (ret, params)
        self.parameters[m.group(2)] = names
        self.signatures[m.group(2)] = (self.ctype(ret, decl, returned=True), [self.ctype(p, decl) for p in params])

    @staticmethod
    def _spell(t):
        return re.sub(r"\s*\*", "*", " ".join(t.split()))

    def ctype(self, t, decl, returned=False):
        """the ctypes form of the C type `t` by the rule of the module docstring"""
        tok = re.findall(r"\w+|\S", t)
        core = [x for x in tok if x != "const"]
        base, stars = (core[0] if core else ""), core[1:]
        structs = dict(self.base.structs, **self.structs) if self.base else self.structs
        opaque = self.opaque | self.base.opaque if self.base else self.opaque
        if any(x != "*" for x in stars) or not (base in _SCALARS or base in _POINTEES or base in structs or base in opaque):
            self._bad("type `%s` is outside the vocabulary" % t, decl)
        if not stars:
            if base == "void" and returned:
                return None
            if base not in _SCALARS:
                self._bad("`%s` by value" % t, decl)
            return _SCALARS[base]
        if tok[-2:] == ["*", "*"]:
            return POINTER(c_void_p)
        if len(stars) == 1 and base == "char" and returned:
            return c_char_p
        if len(stars) == 1 and base in structs:
            return POINTER(structs[base])
        if len(stars) == 1 and base == "int":
            return POINTER(c_int)
        return c_void_p


def read_header(name, base=None):
    """include/<name> of this tree (also for another build of the same ABI, T2V_LIBRARY); base: the Header a companion
    header includes"""
    path = os.path.join(INCLUDE_DIR, name)
    if not os.path.exists(path):
        raise RuntimeError("header %s not found: the binding reads the C ABI from it" % path)
    with open(path) as f:
        return Header(f.read(), name, base)


class Binding:
    """One shared library and the header that declares it.  `first` runs once before the library is opened."""

    def __init__(self, lib_path, header, abi_symbol, abi_macro, what, first=None):
        self.lib_path, self.abi_symbol, self.what, self.first = lib_path, abi_symbol, what, first
        self.header = read_header(header)
        self.signatures, self.abi_version = self.header.signatures, self.header.constants[abi_macro]
        self.prefix = abi_symbol[:-len("_abi_version")]
        self.companions = []      # headers that declare further entry points of the same library (companion())
        self._lib, self._lock = None, threading.RLock()

    def constants(self, prefix):
        """the header's constants that start with `prefix`, without it"""
        return {k[len(prefix):]: v for k, v in self.header.constants.items() if k.startswith(prefix)}

    def companion(self, header):
        """A header that includes this binding's and declares more entry points of the same library, with its types: they are
        bound by load() like the main header's; `signatures` stays the main header's."""
        h = read_header(header, self.header)
        self.companions.append(h)
        return h

    def load(self):
        """Load the library and bind every declared symbol.  Raises if anything is missing."""
        if self._lib is None:
            with self._lock:      # (vid2vid/test.py brings the runtime up on a thread while the main thread still imports)
                if self._lib is None:
                    self._lib = self._load_locked()
        return self._lib

    def _load_locked(self):
        so = os.path.basename(self.lib_path)
        if not os.path.exists(self.lib_path):
            raise RuntimeError("%s not found at %s: %s.  Build it with `python __graft_entry__.py` or "
                               "`make -C text2video_amd/csrc`." % (so, self.lib_path, self.what))
        if self.first:
            self.first()
        lib = ctypes.CDLL(self.lib_path)
        declared = list(self.signatures.items()) + [kv for h in self.companions for kv in h.signatures.items()]
        for name, (res, args) in declared:
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        got = getattr(lib, self.abi_symbol)()
        if got != self.abi_version:
            raise RuntimeError("%s ABI %d != binding ABI %d (include/%s)" % (so, got, self.abi_version, self.header.name))
        return lib

    def check(self, status, what=""):
        if status != 0:
            msg = getattr(self.load(), self.prefix + "_last_error")()
            raise RuntimeError("%s %s failed (status %d): %s" % (self.prefix, what, status, msg.decode() if msg else "?"))


bind = Binding

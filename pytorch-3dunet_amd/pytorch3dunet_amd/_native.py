"""ctypes binding of libu3d_hip.so (gfx950 HIP kernels), derived from include/u3d.h at import — and of the extension library
libu3d_ext_hip.so next to it, derived from include/u3d_ext.h into a third table (`_EXT_PROTOS`) and loaded lazily, on the first call of one
of its names (`get_ext_lib`).

The header — include/u3d.h and the parts it includes (`PART_PATHS`, read by `read_part` into a second table, `_PART_PROTOS`) — is the only
statement of the C-ABI: `parse_header` reads its declarations, the four `typedef struct`s and the `U3D_*`
constants, and this module keeps no second copy of any of them.  One type rule: scalars map through `_SCALARS`; EVERY pointer argument
and struct field is `c_void_p` (struct pointers too: two of the four structs travel as device arrays through `data_ptr()`, so a typed
pointer cannot be the rule), which takes `ctypes.byref(struct)`, `(c_int * n)(...)`, an integer address and None alike; a
`const char*` return is `c_char_p`.  The reader is strict: whatever it does not understand raises `U3DError`, nothing is skipped.

The product path has NO fallback: if the shared library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# (U3D_LIB_PATH: another build of the same library — same-box A/B runs of compile-time kernel experiments, tools/ab_libs.sh)
LIB_PATH = os.environ.get("U3D_LIB_PATH") or os.path.join(_HERE, "lib", "libu3d_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "u3d.h"))


class U3DError(RuntimeError):
    pass


_SCALARS = {"int": c_int, "long long": c_int64, "int64_t": c_int64, "int32_t": c_int32, "size_t": c_size_t, "float": c_float,
            "double": c_double, "u3d_stream_t": c_void_p}
_POINTEES = set(_SCALARS) - {"u3d_stream_t"} | {"void", "uint8_t", "char"}  # + the header's own structs
_STRUCT_NAMES = {"u3d_src_t": "U3DSrc", "u3d_adam_desc_t": "U3DAdamDesc", "u3d_gn_bwd_job_t": "U3DGnBwdJob", "u3d_pack_desc_t": "U3DPackDesc"}
_CONSTANTS = ("U3D_VERSION", "U3D_OK", "U3D_EINVAL", "U3D_EHIP", "U3D_EARCH", "U3D_EWORKSPACE")

_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")  # (the tag, if any, is not used)
_FUNC = re.compile(r"([\w\s*]+?)\b(u3d_[a-z0-9_]+)\s*\(([^(){};]*)\)\s*;")
_STREAM = re.compile(r"typedef\s+void\s*\*\s*u3d_stream_t\s*;")


def _ctype(decl, pointees, where):
    """`[const] base [*] name` -> (ctype, name)"""
    toks = decl.replace("*", " * ").split()
    toks = toks[1:] if toks[:1] == ["const"] else toks
    star = toks[-2:-1] == ["*"]
    base, name = " ".join(toks[:-2 if star else -1]), "".join(toks[-1:])
    if not name.isidentifier() or (base not in pointees if star else base not in _SCALARS):
        raise U3DError(f"u3d.h: unknown type {base + '*' * star!r} of {name!r} in {where}")
    return (c_void_p if star else _SCALARS[base]), name


def parse_header(text):
    """(prototypes {name: (restype, [argtypes])}, structs {C name: [(field, ctype)]}, constants {name: int}) of a u3d.h text, all in
    header order.  Raises U3DError on anything that is not a declaration it understands."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {}
    for line in re.findall(r"^[ \t]*#[ \t]*(.*?)[ \t]*$", text, flags=re.M):
        m = re.fullmatch(r"define[ \t]+(U3D_\w+)(?:[ \t]+(-?\d+|\(-?\d+\)))?", line)  # (no value: the include guard)
        if m and m.group(2) and m.group(1) not in consts:
            consts[m.group(1)] = int(m.group(2).strip("()"))
        elif (m and m.group(2)) or not (m or re.fullmatch(r"ifndef[ \t]+U3D_H|ifdef[ \t]+__cplusplus|endif|include[ \t]*<\w+\.h>", line)):
            raise U3DError(f"u3d.h: #{line}: not the guard, the C++ wrapper, an #include or one integer constant U3D_* defined once")
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, flags=re.S)
    text = _STREAM.sub("", m.group(1) if m else text, count=1)
    structs = {}
    for body, cname in _STRUCT.findall(text):
        if cname in structs:
            raise U3DError(f"u3d.h: struct {cname} is declared twice")
        fields = structs[cname] = []
        for field in filter(None, (f.strip() for f in body.split(";"))):
            first, *more = field.split(",")
            ctype, name = _ctype(first, _POINTEES | set(structs), f"struct {cname}")
            if more and ("*" in first or not all(n.strip().isidentifier() for n in more)):
                raise U3DError(f"u3d.h: cannot parse field {field!r} of struct {cname}")
            fields += [(n.strip(), ctype) for n in (name, *more)]
    text = _STRUCT.sub("", text)
    pointees, protos = _POINTEES | set(structs), {}
    for ret, name, args in _FUNC.findall(text):
        if name in protos:
            raise U3DError(f"u3d.h: {name} is declared twice")
        ret, args = " ".join(ret.split()), args.strip()
        if ret != "const char*" and ret not in _SCALARS:
            raise U3DError(f"u3d.h: unknown return type {ret!r} of {name}")
        argtypes = [] if args in ("", "void") else [_ctype(a, pointees, name)[0] for a in args.split(",")]
        protos[name] = (c_char_p if ret == "const char*" else _SCALARS[ret], argtypes)
    rest = _FUNC.sub("", text).strip()
    if rest:
        m = re.search(r"u3d_[a-z0-9_]+\s*\(", rest)
        raise U3DError(f"u3d.h: not a declaration this reader understands: {(m.group(0) if m else rest[:60])!r}")
    return protos, structs, consts


def read_header(path):
    if not os.path.exists(path):
        raise U3DError(f"C-ABI header {path} not found: the binding is derived from include/u3d.h of the source tree "
                       "(looked for it relative to the package, <package>/../../include/u3d.h).")
    with open(path) as fh:
        protos, structs, consts = parse_header(fh.read())
    if set(structs) != set(_STRUCT_NAMES) or not set(_CONSTANTS) <= set(consts):
        raise U3DError(f"{path}: structs {sorted(structs)} / constants {sorted(consts)} are not the ones this module names")
    return protos, structs, consts


_PROTOS, _structs, _consts = read_header(HEADER_PATH)  # name: (restype, argtypes), in header order
EXPORTED_SYMBOLS = tuple(_PROTOS)


def read_part(path, known):
    """prototypes of a part of the C-ABI that u3d.h includes (`#include <u3d_*.h>` inside its extern "C" block): declarations only, in
    u3d.h's form, read by the same strict reader; a name u3d.h already declares raises"""
    if not os.path.exists(path):
        raise U3DError(f"C-ABI header part {path} not found (include/u3d.h includes it)")
    with open(path) as fh:
        protos, structs, consts = parse_header(fh.read())
    if structs or consts or set(protos) & set(known):
        raise U3DError(f"{path}: a part of u3d.h holds function declarations only, none of them u3d.h's own")
    return protos


# the parts u3d.h includes, in its order: the sub-pixel bf16 entry points of a UNet3D (`bf16_subpixel`)
PART_PATHS = (os.path.join(os.path.dirname(HEADER_PATH), "u3d_subpix_bf16.h"),)
_PART_PROTOS = {}
for _path in PART_PATHS:
    _PART_PROTOS.update(read_part(_path, {**_PROTOS, **_PART_PROTOS}))
PART_SYMBOLS = tuple(_PART_PROTOS)
ALL_SYMBOLS = EXPORTED_SYMBOLS + PART_SYMBOLS  # every u3d_* the library exports: u3d.h's own declarations, then its parts'
# the extension library's C-ABI (include/u3d_ext.h, a header in the form of a part: u3d.h does NOT include it): the 16-channel bf16 entry
# points of a UNet3D (`bf16_stem`), the split weight gradient (`fp32_split_wgrad`) and the 3x3 convolutions of a UNet2D in fp32_split
# (`native_2d_fp32_split`; with the residual epilogue: a ResidualUNet2D's, `native_2d_residual_fp32_split`).  The core's tables above do not know these names; `call` resolves them in `get_ext_lib()`.
EXT_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "u3d_ext.h")
EXT_LIB_PATH = os.environ.get("U3D_EXT_LIB_PATH") or os.path.join(os.path.dirname(LIB_PATH), "libu3d_ext_hip.so")
_EXT_PROTOS = read_part(EXT_HEADER_PATH, {**_PROTOS, **_PART_PROTOS})
EXT_SYMBOLS = tuple(_EXT_PROTOS)
U3D_EXT_VERSION = 2  # what u3d_ext_version() of a matching libu3d_ext_hip.so returns
U3D_VERSION, U3D_OK, U3D_EINVAL, U3D_EHIP, U3D_EARCH, U3D_EWORKSPACE = (_consts[k] for k in _CONSTANTS)
U3DSrc, U3DAdamDesc, U3DGnBwdJob, U3DPackDesc = (
    type(py, (ctypes.Structure,), {"_fields_": _structs[c], "__doc__": f"{c} of include/u3d.h"}) for c, py in _STRUCT_NAMES.items())

_lib = None
_ext_lib = None  # stays None until the first call of an extension name: a model without `bf16_stem` / `fp32_split_wgrad` / `native_2d_fp32_split` never loads the library
_lock = threading.Lock()
launch_count = 0  # number of native calls issued (tests assert the HIP path really ran)


def lib_available() -> bool:
    return os.path.exists(LIB_PATH)


def get_lib():
    """Load libu3d_hip.so (once).  Raises U3DError if it has not been built — there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise U3DError(
                f"native library {LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). The MI355X path has no CPU/PyTorch fallback."
            )
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so): it must be in the process BEFORE this
        # library is loaded so that both share ONE runtime (streams, allocations); loading ours first would pull
        # in /opt/rocm's copy as a second, unusable runtime.
        import torch  # noqa: F401

        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in {**_PROTOS, **_PART_PROTOS}.items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
            fn.restype = res
            fn.argtypes = args
        if lib.u3d_version() < U3D_VERSION:
            raise U3DError("libu3d_hip.so is older than the Python host code")
        for kv in os.environ.get("U3D_TUNE", "").split(","):  # A/B knobs of u3d_set_tuning, e.g. U3D_TUNE=8:256,9:1 (results never change)
            if ":" in kv:
                k, v = kv.split(":")
                if lib.u3d_set_tuning(int(k), int(v)) != 0:
                    raise U3DError(f"U3D_TUNE: bad knob {kv!r}")
        _lib = lib
    return _lib


def get_ext_lib():
    """Load libu3d_ext_hip.so (once, after the core library it links against).  Raises U3DError if it has not been built."""
    global _ext_lib
    if _ext_lib is not None:
        return _ext_lib
    get_lib()
    with _lock:
        if _ext_lib is not None:
            return _ext_lib
        if not os.path.exists(EXT_LIB_PATH):
            raise U3DError(
                f"native extension library {EXT_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). The MI355X path has no CPU/PyTorch fallback."
            )
        lib = ctypes.CDLL(EXT_LIB_PATH)
        for name, (res, args) in _EXT_PROTOS.items():
            fn = getattr(lib, name, None)
            if fn is None:  # (a library from before include/u3d_ext.h gained the name: its version alone would not say so)
                raise U3DError(f"libu3d_ext_hip.so does not export {name}, which include/u3d_ext.h declares: rebuild it "
                               "with `python -c 'import __graft_entry__ as g; g.build()'`")
            fn.restype = res
            fn.argtypes = args
        if lib.u3d_ext_version() != U3D_EXT_VERSION:
            raise U3DError(f"libu3d_ext_hip.so has version {lib.u3d_ext_version()}, the Python host code expects {U3D_EXT_VERSION}: rebuild it "
                           "with `python -c 'import __graft_entry__ as g; g.build()'`")
        _ext_lib = lib
    return _ext_lib


def check(rc: int, what: str = "") -> None:
    if rc != U3D_OK:
        msg = get_lib().u3d_last_error()
        raise U3DError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


class EventProfiler:
    """Per-entry-point device time from HIP events recorded on the launching stream (bench.py's roofline leg).
    Usage: nat.profiler = EventProfiler(); ...run...; torch.cuda.synchronize(); prof.summary()."""

    def __init__(self, flops_only: bool = False, only=None, prealloc: int = 0):
        import torch

        # creating a timing event costs ~0.1-0.2 ms of HOST time the first time (hipEventCreate; torch only pools events it has seen
        # freed): a timed region that creates ~50 events per step becomes host-bound (measured: 3.3 -> 12.4 ms of host time per
        # step, 17.5 -> 20 ms per step).  `prealloc` events are therefore created up front, outside any timed region.
        self._pool = [torch.cuda.Event(enable_timing=True) for _ in range(int(prealloc))]
        for ev in self._pool:
            ev.record()  # torch creates the HIP event lazily, at the first record(): force it NOW (measured: with few warm-up steps the
                         # timed region otherwise paid ~75 ms of event creation, 17.4 -> 24 ms per step at --steps 10 --warmup 1..3)
        if self._pool:
            torch.cuda.synchronize()
        self.records = []  # (name, flops, start_event, end_event)
        self.only = set(only) if only else None  # bracket just these entry points (bench.py: the dominant family in the timed region)
        # flops_only: time only the MFMA families (calls that declare FLOPs) — two event packets per call cost ~1 us of
        # device time each, 0.7 ms per step when every one of the ~320 calls is bracketed
        self.flops_only = flops_only

    def wrap(self, name, fn, args, flops):
        import torch

        if (self.flops_only and flops <= 0.0) or (self.only is not None and name not in self.only):
            return fn(*args)
        st = self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)
        en = self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)
        st.record()
        rc = fn(*args)
        en.record()
        self.records.append((name, flops, st, en))
        return rc

    def summary(self):
        out = {}
        for name, flops, st, en in self.records:
            d = out.setdefault(name, {"calls": 0, "ms": 0.0, "flops": 0.0})
            d["calls"] += 1
            d["ms"] += st.elapsed_time(en)
            d["flops"] += flops
        return out


profiler = None


def call(name: str, *args, flops: float = 0.0) -> None:
    """Call an int-returning entry point and raise on error."""
    global launch_count
    fn = getattr(get_ext_lib() if name in _EXT_PROTOS else get_lib(), name)
    launch_count += 1
    rc = fn(*args) if profiler is None else profiler.wrap(name, fn, args, flops)
    if rc != U3D_OK:
        check(rc, name)
